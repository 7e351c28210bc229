"""The KITTI-protocol table on the device (evaluate.dataset_ap.kitti: dpft_dataset_ap_update_kitti_f32,
dpft_dataset_ap_finalize_kitti_f64 / _groups_f64) against the literal two passes of tests/dataset_ap_kitti_ref.py.

* records: bits 8..15 of the fourth word (pass 1) equal the reference's bit for bit; bits 16..23 (pass 2) are compared as sums
  up to the end of every score tie group of a frame -- inside a tie group the single bits depend on the insertion order, their
  sum does not;
* thresholds, nthr, tp and fp are equal exactly (scores are fp32 values, counts are integers);
* prec, rec, AP and AP11 within AP_TOL = 1e-12 of tests/test_gpu_dataset_ap.py (correctly rounded quotients of exact integers,
  at most 41 terms in [0, 1] summed in the same order).
Every case is checked by the reference's ``violations`` first: no IoU near a threshold, no near-tie of two different boxes on one
target."""
import functools

import numpy as np
import pytest
import torch

from tests import dataset_ap_kitti_ref as KR
from tests import dataset_ap_ref as R
from tests.test_gpu_dataset_ap import AP_TOL, DEV, _batch, _same

pytestmark = pytest.mark.gpu

K1 = {"kinds": ("bev",), "iou": (0.3,)}
K5 = {"kinds": ("3d",), "iou": (0.1, 0.2, 0.3, 0.5, 0.7)}
K6, K8 = R.K6, R.K8


# ----------------------------------------------------------------------------------------------------------------- cases
def _dense_sample(rng, N, m, C, jitter=0.25, copies=0.7):
    """Like dataset_ap_ref.random_sample, but every query is a detection (class != 0, centre inside the roi): D = N."""
    f32 = np.float32
    s = R.random_sample(rng, N, m, C)
    label = rng.integers(1, C, N)
    gt_id = np.argmax(s["gt_class"], 1) if m else np.zeros(0, dtype=np.int64)
    for n in range(N):
        if m and rng.uniform() < copies:
            j = int(rng.integers(0, m))
            s["center"][n] = s["gt_center"][j] + rng.normal(0, jitter, 3).astype(f32)
            s["size"][n] = np.maximum(s["gt_size"][j] * rng.uniform(0.8, 1.25, 3).astype(f32), f32(0.5))
            s["angle"][n] = s["gt_angle"][j] + rng.normal(0, 0.05, 2).astype(f32)
            if gt_id[j] != 0 and rng.uniform() < 0.85:
                label[n] = gt_id[j]
    s["center"][:, 0] = np.clip(s["center"][:, 0], 1.0, 71.0)
    s["center"][:, 1] = np.clip(s["center"][:, 1], -6.0, 6.0)
    s["center"][:, 2] = np.clip(s["center"][:, 2], -1.5, 5.5)
    cls = rng.normal(0, 0.1, (N, C)).astype(f32) - f32(1.0)
    cls[np.arange(N), label] = rng.uniform(0.01, 1.0, N).astype(f32)
    s["cls"] = cls
    return s


def _box(x, y, z=0.0, l=4.0, w=2.0, h=1.5, s=0.0, c=1.0):
    return (x, y, z, l, w, h, s, c)


def _pairs_frame(rng, n_pairs, n_false, tie_every=0):
    """n_pairs isolated 2 m x 1 m targets on a 3 m x 2 m grid, each with one detection shifted by a few centimetres (always
    matched at bev 0.3), and n_false detections on free grid cells; class 1 of 2.  tie_every = t: every t-th matched detection
    repeats the score of the one before it."""
    cells = [(4.0 + 3.0 * i, -5.0 + 2.0 * j) for i in range(22) for j in range(6)]
    order = rng.permutation(len(cells))
    assert n_pairs + n_false <= len(cells)
    gts, dets = [], []
    scores = rng.permutation(np.arange(1, 1001))[:n_pairs + n_false].astype(np.float32) / np.float32(1024.0)
    for p in range(n_pairs):
        x, y = cells[order[p]]
        gts.append((1, _box(x, y, l=2.0, w=1.0)))
        s = float(scores[p]) if not (tie_every and p % tie_every == tie_every - 1) else dets[-1][1]
        dets.append((1, s, _box(x + float(rng.uniform(-0.2, 0.2)), y + float(rng.uniform(-0.1, 0.1)), l=2.0, w=1.0)))
    for p in range(n_pairs, n_pairs + n_false):
        x, y = cells[order[p]]
        dets.append((1, float(scores[p]), _box(x, y, l=2.0, w=1.0)))
    mix = rng.permutation(len(dets))
    return R.hand_sample([dets[i] for i in mix], gts, 2)


def _chain_frame():
    """Targets at x = 10, 11, 12 (4 m x 2 m, overlapping on purpose).  a (0.9, x = 10.6) goes to t0, b (0.8, x = 11.7) to t1; c
    (0.7, x = 10) then takes t0 from a, a takes t1 from b, b goes to the free t2: three targets change hands in one insertion."""
    dets = [(1, 0.9, _box(10.6, 0)), (1, 0.8, _box(11.7, 0)), (1, 0.7, _box(10.0, 0)), (1, 0.6, _box(40.0, 3.0))]
    gts = [(1, _box(10.0, 0)), (1, _box(11.0, 0)), (1, _box(12.0, 0)), (1, _box(60.0, -3.0))]
    return R.hand_sample(dets, gts, 2)


def _tie_frame(flip=False):
    """Queries 0 and 1 are the same box with the same score (equal IoU, equal score), 2 the same box with a higher score (equal
    IoU), 3 and 4 share a second target, 5 overlaps nothing, 6 is of class 2 which has no target; the target at x = 60 is reached
    by nothing, and neither is the only target of class 3 (targets and no pass-1 TP: n1 = 0)."""
    dets = [(1, 0.5, _box(10.2, 0)), (1, 0.5, _box(10.2, 0)), (1, 0.75, _box(10.2, 0)), (1, 0.5, _box(20.1, 0)),
            (1, 0.25, _box(20.05, 0.1)), (1, 0.5, _box(40.0, 2.0)), (2, 0.5, _box(30.0, 0))]
    gts = [(1, _box(10.0, 0)), (1, _box(20.0, 0)), (1, _box(60.0, 0)), (3, _box(50.0, 0))]
    return R.hand_sample(dets[::-1] if flip else dets, gts[::-1] if flip else gts, 4)


def _negative_frame():
    """Negative scores are detections under min_score = -1 (the other logits lie at -5): pass 1 passes them over."""
    s = R.hand_sample([(1, -0.5, _box(10.1, 0)), (1, 0.25, _box(20.1, 0)), (1, -0.25, _box(20.0, 0.1)), (1, -0.0, _box(30.1, 0))],
                      [(1, _box(10.0, 0)), (1, _box(20.0, 0)), (1, _box(30.0, 0))], 2)
    for n in range(4):
        s["cls"][n, 0] = -5.0
    return s


@functools.lru_cache(maxsize=None)
def _exact_g():
    """The smallest G >= 200 at which the sampling loop with n1 = G meets (r - cur) == (cur - l) exactly, found in the reference."""
    for G in range(200, 400):
        notes = {}
        KR.pick_thresholds([1.0] * G, G, notes)
        if notes.get("exact"):
            return G
    raise AssertionError("no G in 200..399 hits the equality")


def _frames(name, attempt=0):
    """name -> (frames, num_classes, params); ``attempt`` moves the seed of a random case."""
    rng = np.random.default_rng(sum(ord(ch) for ch in name) + 7919 * attempt)
    if name == "chain":
        return [(5, _chain_frame())], 2, dict(K6)
    if name == "ties":                     # equal scores across frames 7, 8, 9: 0.5 is a threshold and its tie group spans them
        return [(7, _tie_frame()), (8, _tie_frame(flip=True)), (9, _tie_frame())], 4, dict(K6)
    if name == "negative":
        return [(0, _negative_frame())], 2, dict(K6, min_score=-1.0)
    if name == "d64_m64_k1":
        return [(3, _dense_sample(rng, 64, 64, 2))], 2, dict(K1)
    if name == "d65_m65_k5":
        return [(3, _dense_sample(rng, 65, 65, 3)), (4, _dense_sample(rng, 65, 10, 3)), (5, _dense_sample(rng, 65, 0, 3))], 3, dict(K5)
    if name == "d100_m256_k8":
        return [(0, _dense_sample(rng, 100, 256, 4))], 4, dict(K8)
    if name == "d1024_one_target":         # every one of the 1024 detections lies above the threshold of the only target
        s = _dense_sample(rng, 1024, 1, 2, copies=1.0)
        s["gt_class"][0] = (0.0, 1.0)
        s["gt_size"][0], s["gt_angle"][0], s["gt_center"][0] = (4.0, 2.0, 1.5), (0.0, 1.0), (20.0, 0.0, 0.0)
        s["center"][:] = s["gt_center"][0] + np.concatenate([rng.uniform(-0.3, 0.3, (1024, 2)), np.zeros((1024, 1))], 1).astype(np.float32)
        s["size"][:], s["angle"][:] = s["gt_size"][0], s["gt_angle"][0]
        s["cls"][:, 1] = (rng.permutation(1024) + 1).astype(np.float32) / np.float32(2048.0)
        return [(0, s)], 2, dict(K1)
    if name == "n1_40":
        return [(0, _pairs_frame(rng, 40, 9))], 2, dict(K1)
    if name == "n1_41":
        return [(0, _pairs_frame(rng, 41, 9, tie_every=5))], 2, dict(K1)
    if name == "n1_exact":                 # n1 = G = a few hundred, at a G where the sampling loop meets its equality
        G = _exact_g()
        per = [G // 4, G // 4, G // 4, G - 3 * (G // 4)]
        return [(20 + f, _pairs_frame(rng, per[f], 12 + max(per) - per[f], tie_every=7)) for f in range(4)], 2, dict(K1)      # (one N)
    if name == "stream":                   # 8 small crowded frames for the batch-split, merge and group tests
        return [(100 + f, _dense_sample(rng, 24, int(rng.integers(0, 7)), 3, jitter=0.4)) for f in range(8)], 3, dict(K6)
    raise KeyError(name)


CASES = ("chain", "ties", "negative", "d64_m64_k1", "d65_m65_k5", "d100_m256_k8", "d1024_one_target", "n1_40", "n1_41", "n1_exact",
         "stream")


@functools.lru_cache(maxsize=None)
def _case(name):
    """(frames, num_classes, params, reference, notes); a random case is redrawn (never dropped) until it is safe to compare."""
    for attempt in range(50):
        frames, C, params = _frames(name, attempt)
        notes = {}
        ref = KR.run(frames, C, notes=notes, **params)
        bad = KR.violations(ref["prepared"], ref["combos"])
        if not bad:
            return frames, C, params, ref, notes
        assert name not in ("chain", "ties", "negative"), bad                # the hand-made cases must be safe as they are
    raise AssertionError(f"{name}: no safe draw in 50 attempts")


# --------------------------------------------------------------------------------------------------------------- helpers
def _new(C, params, **kw):
    from dpft_amd.evaluation.dataset_ap import DatasetAP
    return DatasetAP(C, **params, **kw)


def _feed(ap, frames, sizes=None, descriptions=None):
    """Updates of at most 4 consecutive frames (``sizes``: the batch split)."""
    sizes = sizes or [min(4, len(frames) - i) for i in range(0, len(frames), 4)]
    assert sum(sizes) == len(frames) and max(sizes) <= 4
    i = 0
    for n in sizes:
        chunk = frames[i:i + n]
        assert [f for f, _ in chunk] == list(range(chunk[0][0], chunk[0][0] + n))
        out, labels = _batch([s for _, s in chunk])
        if descriptions is not None:
            for lab, d in zip(labels, descriptions[i:i + n]):
                lab["description"] = torch.tensor(d, dtype=torch.float32, device=DEV)
        ap.update(out, labels, chunk[0][0])
        i += n


def _raw(ap):
    """The store's records as [score bits, frame, query, class, word 3] in the reference's order."""
    rec = ap.state()["records"].cpu().numpy()
    score = rec[:, 0].copy().view(np.float32).astype(np.float64)
    cols = np.stack([rec[:, 0], rec[:, 1], rec[:, 2] & 0xFFFF, (rec[:, 2] >> 16) & 0xFF, rec[:, 3]], 1).astype(np.int64)
    return cols[np.lexsort((cols[:, 2], cols[:, 1], -score, cols[:, 3]))]


def _check_bits(ap, ref):
    got = _raw(ap)
    want = ref["records"]
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got[:, :4], want[:, :4])
    assert np.array_equal((got[:, 4] >> 8) & 0xFF, want[:, 4]), np.argwhere(((got[:, 4] >> 8) & 0xFF) != want[:, 4])[:5]
    assert not np.any(got[:, 4] >> 24)
    K = len(ref["combos"])
    score = got[:, 0].astype(np.int32).view(np.float32).astype(np.float64)
    seen = 0
    for f in np.unique(got[:, 1]):
        for c in np.unique(got[got[:, 1] == f, 3]):
            rows = np.flatnonzero((got[:, 1] == f) & (got[:, 3] == c))          # already by score descending
            running = np.zeros(K, dtype=np.int64)
            for p, r in enumerate(rows):
                running += (got[r, 4] >> (16 + np.arange(K))) & 1
                if p + 1 == len(rows) or score[rows[p + 1]] != score[r]:        # the end of a score tie group of the frame
                    assert running.tolist() == ref["tiesums"][(int(f), int(c), float(score[r]))], (f, c, score[r])
                    seen += 1
    assert seen == len(ref["tiesums"])


def _check_table(res, ref, C):
    for key in ("thresholds", "tp", "fp"):
        assert np.array_equal(res[f"kitti_{key}"].numpy(), ref[key], equal_nan=True), key
    assert np.array_equal(res["kitti_nthr"].numpy(), ref["nthr"])
    assert _same(res["npos"], ref["npos"])
    for key, name in (("prec", "kitti_prec"), ("rec", "kitti_rec"), ("ap", "kitti_ap"), ("ap11", "kitti_ap11")):
        err = np.nanmax(np.abs(res[name].numpy() - ref[key]), initial=0.0)
        print(f"max |{name} - ref| =", err)
        assert _same(res[name], ref[key], AP_TOL), (key, err)
    for k, (kind, thr) in enumerate(ref["combos"]):
        assert _same(res[f"kitti/mAP_{kind}@{thr:g}"], ref["mAP"][k], AP_TOL)
        assert _same(res[f"kitti/mAP11_{kind}@{thr:g}"], ref["mAP11"][k], AP_TOL)
        for c in range(1, C):
            assert _same(res[f"kitti/AP_{kind}@{thr:g}/{c}"], ref["ap"][c - 1, k], AP_TOL)
            assert _same(res[f"kitti/AP11_{kind}@{thr:g}/{c}"], ref["ap11"][c - 1, k], AP_TOL)


def _run(name, **kw):
    frames, C, params, ref, notes = _case(name)
    ap = _new(C, params, kitti=True, **kw)
    _feed(ap, frames)
    return ap, frames, C, params, ref, notes


# ----------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", CASES)
def test_bits_and_table_equal_the_literal_two_passes(name):
    ap, frames, C, params, ref, notes = _run(name)
    _check_bits(ap, ref)
    _check_table(ap.compute(), ref, C)


def test_the_cases_reach_what_they_are_for():
    """The properties the cases were built for, asserted in the reference alone."""
    _, _, _, ref, _ = _case("chain")
    notes = {}
    KR.frame_bits(ref["prepared"][0], 1, 0, 0.3, notes)
    assert notes["chain"] == 3
    assert ref["npos"].tolist() == [4.0] and ref["tp"][0, 0, :ref["nthr"][0, 0]].max() == 3      # the target at x = 60 stays free
    _, _, _, ref, _ = _case("ties")
    assert 0.5 in ref["thresholds"][0, 0].tolist() and ref["npos"].tolist() == [9.0, 0.0, 3.0]
    assert len({int(r[1]) for r in ref["records"] if r[3] == 1 and r[0] == R.score_bits(0.5)}) == 3
    assert np.isnan(ref["ap"][1]).all() and ref["nthr"][1].tolist() == [0] * 6                   # npos = 0
    assert ref["ap"][2].tolist() == [0.0] * 6 and ref["nthr"][2].tolist() == [0] * 6             # n1 = 0 with targets
    _, _, _, ref, _ = _case("negative")
    assert ref["nthr"][0, 0] == 2 and ref["thresholds"][0, 0, :2].tolist() == [0.25, 0.0] and ref["records"][:, 4].tolist() == [63, 63, 0, 0]
    for name, D, M in (("d64_m64_k1", 64, 64), ("d65_m65_k5", 65, 65), ("d100_m256_k8", 100, 256), ("d1024_one_target", 1024, 1)):
        _, _, _, ref, _ = _case(name)
        fr = ref["prepared"][0]
        assert len(fr["dets"]) == D and fr["sample"]["gt_class"].shape[0] == M, name
    fr = _case("d1024_one_target")[3]["prepared"][0]
    assert sum(v[0] > 0.3 for v in fr["iou"].values()) == 1024
    assert _case("n1_40")[3]["nthr"][0, 0] == 40 and _case("n1_40")[3]["npos"][0] == 40
    assert _case("n1_41")[3]["nthr"][0, 0] == 41 and _case("n1_41")[3]["npos"][0] == 41
    _, _, _, ref, notes = _case("n1_exact")
    assert notes["exact"][(1, 0)] >= 1 and ref["npos"][0] == _exact_g() >= 200 and ref["nthr"][0, 0] == 41
    assert int((ref["records"][:, 4] & 1).sum()) == _exact_g()                                    # n1 = G


def test_another_batch_split_and_a_merge_give_the_same_bits():
    frames, C, params, ref, _ = _case("stream")
    whole = _new(C, params, kitti=True)
    _feed(whole, frames, [4, 4])
    split = _new(C, params, kitti=True, initial_capacity=32)
    _feed(split, frames, [1, 3, 2, 2])
    a, b = _new(C, params, kitti=True), _new(C, params, kitti=True)
    _feed(a, frames[:3], [3])
    _feed(b, frames[3:], [4, 1])
    a.merge(b)
    want = _raw(whole)
    res = whole.compute()
    for other in (split, a):
        assert np.array_equal(_raw(other), want)
        got = other.compute()
        for key in ("kitti_ap", "kitti_ap11", "kitti_prec", "kitti_rec", "kitti_thresholds", "kitti_tp", "kitti_fp", "kitti_nthr", "ap"):
            assert np.array_equal(got[key].numpy(), res[key].numpy(), equal_nan=True), key
    _check_bits(a, ref)
    _check_table(a.compute(), ref, C)


def test_without_the_key_bits_8_to_23_are_zero_and_the_voc_table_is_the_same():
    frames, C, params, ref, _ = _case("stream")
    plain, kitti = _new(C, params), _new(C, params, kitti=True)
    _feed(plain, frames)
    _feed(kitti, frames)
    p, k = _raw(plain), _raw(kitti)
    assert not np.any(p[:, 4] >> 8) and np.any(k[:, 4] >> 8)
    assert np.array_equal(p[:, :4], k[:, :4]) and np.array_equal(p[:, 4], k[:, 4] & 0xFF)
    rp, rk = plain.compute(), kitti.compute()
    assert not [key for key in rp if "kitti" in key]
    for key in rp:
        assert _same(rp[key], rk[key]) if not isinstance(rp[key], list) else rp[key] == rk[key], key
    assert torch.equal(plain.state()["counters"], kitti.state()["counters"])


def _descriptions(n):
    return [[f % 3, (f // 2) % 2, f % 5] for f in range(n)]                  # [road, time, weather]


def test_every_group_has_the_table_of_an_ungrouped_run_over_its_frames():
    frames, C, params, ref, _ = _case("stream")
    desc = _descriptions(len(frames))
    ap = _new(C, params, kitti=True, groups=["time"])
    _feed(ap, frames, [3, 1, 4], desc)
    res = ap.compute()
    _check_bits(ap, ref)
    _check_table(res, ref, C)                                               # the keys without a group are the ``all`` group's
    values = {name: v for v, name in ap.axis_tables["time"]}
    assert res["group_names"] == ["all"] + [f"time={n}" for _, n in ap.axis_tables["time"]] and len(res["group_names"]) == 3
    for g, gname in enumerate(res["group_names"]):
        member = [i for i in range(len(frames)) if g == 0 or desc[i][1] == values[gname.split("=")[1]]]
        assert 0 < len(member) <= len(frames)
        alone = _new(C, params, kitti=True)
        for i in member:                                                    # (one frame per update: the indices have gaps)
            _feed(alone, [frames[i]], [1])
        want = alone.compute()
        assert np.array_equal(res["group_kitti_ap"][g].numpy(), want["kitti_ap"].numpy(), equal_nan=True), gname
        assert np.array_equal(res["group_kitti_ap11"][g].numpy(), want["kitti_ap11"].numpy(), equal_nan=True), gname
        if g:
            for key, v in want.items():
                if key.startswith("kitti/"):
                    assert _same(res[f"{key}/{gname}"], v), (key, gname)
        sub = KR.run([frames[i] for i in member], C, **params)
        assert _same(want["kitti_ap"], sub["ap"], AP_TOL) and _same(want["kitti_ap11"], sub["ap11"], AP_TOL)


def test_tp_errors_and_groups_together_with_the_key():
    frames, C, params, ref, _ = _case("stream")
    desc = _descriptions(len(frames))
    both = _new(C, params, kitti=True, groups=["time", "road"], tp_errors=True)
    base = _new(C, params, groups=["time", "road"], tp_errors=True)
    _feed(both, frames, [4, 4], desc)
    _feed(base, frames, [4, 4], desc)
    _check_bits(both, ref)
    res, want = both.compute(), base.compute()
    _check_table(res, ref, C)
    sa, sb = both.state(), base.state()                                     # (the store's order is arbitrary: compare in sorted order)
    pa, pb = both.sort_permutation(sa["records"]), base.sort_permutation(sb["records"])
    assert torch.equal(sa["tp_errors"][pa], sb["tp_errors"][pb]) and torch.equal(sa["frames"], sb["frames"])
    assert torch.equal(sa["records"][pa][:, :3], sb["records"][pb][:, :3])
    assert torch.equal(sa["records"][pa][:, 3] & 0xFF, sb["records"][pb][:, 3])
    for key, v in want.items():                                             # everything the run without the key gives, to the bit
        assert (res[key] == v) if isinstance(v, list) else _same(res[key], v), key
    assert res["group_kitti_ap"].shape == (len(res["group_names"]), C - 1, len(ref["combos"]))
    only = _new(C, params, kitti=True, tp_errors=True)                      # tp_errors without groups through the same entry
    _feed(only, frames)
    _check_bits(only, ref)
    assert _same(only.compute()["tp_err"], want["tp_err"])


def test_the_evaluator_logs_the_new_scalars_and_every_condition_repeats_them():
    """Nothing but the config key: the evaluation loop returns ``kitti/...`` beside the other scalars, logs them under ``test/``, and
    a robustness condition repeats each as ``{key}/cond={name}`` after the group suffix."""
    from dpft_amd.evaluation import DataParallelEvaluator
    from dpft_amd.evaluation.dataset_ap import DatasetAP
    from dpft_amd.evaluation.robustness import RobustnessSuite
    from tests import test_gpu_robustness as T
    from tests.test_gpu_dataset_ap import _Writer
    spec = {"conditions": {k: T.CONDITIONS[k] for k in ("nothing", "camera_off")}, "seed": 5}
    ev = DataParallelEvaluator(metric=T._metric, device=DEV, logging="epoch", robustness=RobustnessSuite(spec),
                               dataset_ap=DatasetAP(T.C4, groups=["weather"], kitti=True, **T.AP))
    w = _Writer()
    scalars = ev.evaluate_one_epoch(0, T._InputDrivenModel(), T._loader([(0, 4), (4, 6)]), w, None, shard_start=0)
    clean = {k for k in scalars if k.startswith("kitti/") and "/cond=" not in k}
    names = [f"{kind}@{thr:g}" for kind in T.AP["kinds"] for thr in T.AP["iou"]]
    plain = {f"kitti/{a}_{n}/{c}" for a in ("AP", "AP11") for n in names for c in range(1, T.C4)} | \
        {f"kitti/{a}_{n}" for a in ("mAP", "mAP11") for n in names}
    groups = ev.dataset_ap.group_names[1:]
    assert groups and clean == plain | {f"{k}/{g}" for k in plain for g in groups}
    for name in spec["conditions"]:
        assert {k for k in scalars if k.startswith("kitti/") and k.endswith(f"/cond={name}")} == {f"{k}/cond={name}" for k in clean}
    assert all(f"test/{k}" in w.tags for k in clean) and f"test/kitti/mAP_{names[0]}/{groups[0]}/cond=nothing" in w.tags
    for k in clean:                                                         # zero severity: the clean table to the bit
        assert _same(scalars[k], scalars[f"{k}/cond=nothing"]), k
    assert any(scalars[k] != scalars[f"{k}/cond=camera_off"] for k in plain if scalars[k] == scalars[k])
    assert any(scalars[k] > 0 for k in plain if scalars[k] == scalars[k])
