"""True-positive errors beside the split-level AP on the device (evaluate.dataset_ap.tp_errors: dpft_dataset_ap_update_tp_f32,
dpft_dataset_ap_finalize_tp_f64 and their groups forms) against the restatement of tests/dataset_ap_tp_ref.py.

What must hold, and why the bounds are what they are:
* the records, counters and every result of an accumulator WITHOUT the key are there bit for bit (the same walk writes them);
* the stored integers equal the restatement's: aze and ase exactly (only correctly rounded operations in a fixed order), ate and
  aoe within 1 unit of 2^-32 (sqrt / hypot / atan2 do not promise their last bit on either side); a non-TP row is zeros;
* the final values follow from the stored integers: fed the DEVICE's integers, the restatement's point rule gives the device's
  tp_err bit for bit, all four columns, and tp_points exactly; against the restatement's own integers AZE and ASE are bit for bit
  and ATE and AOE within 2^-32 (a mean of cumulative means of values each off by at most one unit is off by at most one unit);
* growing the stores, the order of the updates, merge and load_state do not move a bit; a group equals, bit for bit, an ungrouped
  accumulator fed the group's frames alone.
The shapes are those of tests/test_gpu_dataset_ap.py (N = 1 .. 1024, up to 256 targets per sample, K = 1, 6, 8) and the groups
stream case (522 records in one class: two trip boundaries of the finalize scan)."""
import copy

import numpy as np
import pytest
import torch

from tests import dataset_ap_groups_ref as G
from tests import dataset_ap_ref as R
from tests import dataset_ap_tp_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
UNIT = 2.0 ** -32
PERIODS = ("2pi", "pi")


def _batch(samples, descriptions=None):
    out = {k: torch.from_numpy(np.stack([s[src] for s in samples])).to(DEV)
           for k, src in (("class", "cls"), ("center", "center"), ("size", "size"), ("angle", "angle"))}
    labels = [{k: torch.from_numpy(s[k]).to(DEV) for k in ("gt_center", "gt_size", "gt_angle", "gt_class")} for s in samples]
    if descriptions is not None:
        for lab, d in zip(labels, descriptions):
            lab["description"] = torch.from_numpy(np.asarray(d, dtype=np.float32))      # on the host, as the dataset delivers them
    return out, labels


def _feed(ap, frames, descriptions=None, only=None):
    """One update per run of consecutive frame indices (of the frames at the positions ``only``, when given)."""
    pos = list(range(len(frames))) if only is None else list(only)
    i = 0
    while i < len(pos):
        j = i + 1
        while j < len(pos) and frames[pos[j]][0] == frames[pos[j - 1]][0] + 1:
            j += 1
        out, labels = _batch([frames[p][1] for p in pos[i:j]], None if descriptions is None else [descriptions[p] for p in pos[i:j]])
        ap.update(out, labels, frames[pos[i]][0])
        i = j


def _new(C, params, **kw):
    from dpft_amd.evaluation.dataset_ap import DatasetAP
    return DatasetAP(C, **params, **kw)


def _ordered(ap):
    """The store's records in the reference's order and layout, and the rows that travel beside them in the same order."""
    st = ap.state()
    rec = st["records"].cpu().numpy()
    score = rec[:, 0].copy().view(np.float32).astype(np.float64)
    cols = np.stack([rec[:, 0], rec[:, 1], rec[:, 2] & 0xFFFF, (rec[:, 2] >> 16) & 0xFF, rec[:, 3]], 1).astype(np.int64)
    order = np.lexsort((cols[:, 2], cols[:, 1], -score, cols[:, 3]))
    rows = st["tp_errors"].cpu().numpy()[order] if "tp_errors" in st else None
    return cols[order], rows


def _bits(t):
    return torch.as_tensor(t, dtype=torch.float64).contiguous().view(torch.int64)


def _same_bits(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and torch.equal(a, b)


def _close(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= tol)))


def _check_rows(ap, ref):
    """The stored integers against the restatement's; returns (records, rows) in the reference's order."""
    cols, rows = _ordered(ap)
    assert rows.shape == ref["rows"].shape and rows.dtype == np.int64, (rows.shape, ref["rows"].shape)
    assert np.array_equal(cols[:, 4], ref["bits"]) and np.array_equal(cols[:, 3], ref["classes"])
    diff = np.abs(rows - ref["rows"])
    print("max |q - ref| per column =", diff.max(0, initial=0))
    assert np.array_equal(rows[:, 1:3], ref["rows"][:, 1:3]), np.argwhere(diff[:, 1:3] != 0)[:5]
    assert diff[:, 0].max(initial=0) <= 1 and diff[:, 3].max(initial=0) <= 1, diff.max(0)
    assert not rows[~ref["flags"]].any()                                    # a non-TP row is zeros
    return cols, rows


def _check_table(res, cols, rows, ref, tp_err, tp_points, npos, recall_points, first_point, tail=""):
    """One table (``tail`` = its group suffix) against the restatement and against the device's own integers."""
    C = len(npos) + 1
    flags = (cols[:, 4] >> ref["k"]) & 1 == 1
    mine_err, mine_points = T.from_rows(cols[:, 3], flags, rows, npos, recall_points, first_point)
    assert _same_bits(tp_err, mine_err), (tail, tp_err, mine_err)          # follows from the stored integers, all four columns
    want_err, want_points = T.from_rows(ref["classes"], ref["flags"], ref["rows"], npos, recall_points, first_point)
    assert np.array_equal(np.asarray(tp_points), want_points) and np.array_equal(mine_points, want_points), (tail, tp_points, want_points)
    err = np.nanmax(np.abs(np.asarray(tp_err) - want_err), initial=0.0)
    print(f"max |tp_err - ref|{tail} =", err)
    assert _same_bits(np.asarray(tp_err)[:, 1:3].copy(), want_err[:, 1:3].copy()), (tail, tp_err, want_err)      # AZE, ASE
    assert _close(np.asarray(tp_err)[:, (0, 3)], want_err[:, (0, 3)], UNIT), (tail, err)                          # ATE, AOE
    for e, name in enumerate(T.NAMES):
        vals = [float(tp_err[c][e]) for c in range(C - 1) if not np.isnan(float(tp_err[c][e]))]
        assert _same_bits(res[f"m{name}{tail}"], sum(vals) / len(vals) if vals else T.NAN), (name, tail)
        for c in range(1, C):
            assert _same_bits(res[f"{name}/{c}{tail}"], float(tp_err[c - 1][e]))
    for c in range(1, C):
        assert res[f"tp_points/{c}{tail}"] == want_points[c - 1]
    return want_err, want_points


def _check_plain(ap, plain):
    """Everything an accumulator without the key gives is there, bit for bit."""
    a, _ = _ordered(ap)
    b, _ = _ordered(plain)
    assert np.array_equal(a, b)
    ca, cb = ap.state()["counters"].cpu(), plain.state()["counters"].cpu()
    cb[3] = ca[3]                                                           # (the one new counter)
    assert torch.equal(ca, cb)
    mine, theirs = ap.compute(), plain.compute()
    assert set(theirs) < set(mine)
    for k, v in theirs.items():
        assert (mine[k] == v) if isinstance(v, list) else _same_bits(mine[k], v), k
    return mine


def _run(frames, C, params, at, period, min_recalls=(0, 0.1), plain=None):
    """One accumulator per ``min_recall`` (the later ones by load_state: the rows do not depend on it), each checked in full."""
    ref = T.run(frames, C, at=at, min_recall=0, angle_period=period, **params)
    if plain is None:
        plain = _new(C, params)
        _feed(plain, frames)
    first, out = None, []
    for m in min_recalls:
        spec = {"min_recall": m, "angle_period": period}
        if at is not None:
            spec["at"] = list(at)
        ap = _new(C, params, tp_errors=spec)
        if first is None:
            _feed(ap, frames)
            first = ap
        else:
            ap.load_state(first.state())
        cols, rows = _check_rows(ap, ref)
        res = _check_plain(ap, plain)
        assert res["tp_saturated"] == ref["saturated"] == 0
        _check_table(res, cols, rows, ref, res["tp_err"], res["tp_points"], ref["npos"], ap.recall_points, T.i_min(m, ap.recall_points))
        out.append((ap, res, ref))
    return out


def _bit_cases():
    """(shape, bit of the reference combination): the first, a middle and the last bit of every shape's K combinations."""
    out = []
    for name in sorted(R.SHAPES):
        K = len(R.combinations(R.SHAPES[name][3]["kinds"], R.SHAPES[name][3]["iou"]))
        out += [(name, k) for k in sorted({0, K // 2, K - 1})]
    return out


@pytest.mark.parametrize("name, k", _bit_cases())
def test_rows_and_table_equal_the_restatement_over_the_shapes(name, k):
    """Both periods, min_recall 0 and 0.1 (n65_m256_c8_k1_r40 serves no point at 0.1: its numbers are compared at 0)."""
    frames, C, params, _ = R.shape_case(name)
    combos = R.combinations(params["kinds"], params["iou"])
    plain = _new(C, params)
    _feed(plain, frames)
    for period in PERIODS:
        for ap, res, ref in _run(frames, C, params, combos[k], period, plain=plain):
            assert ap.tp["k"] == k and ref["k"] == k


def test_the_default_reference_combination_is_the_loosest_of_the_first_kind():
    frames, C, params, _ = R.shape_case("n3_m5_c8_k6_r11")
    (ap, res, ref), = _run(frames, C, params, None, "2pi", min_recalls=(0.1,))
    assert ap.tp["at"] == ("bev", 0.3) and ref["k"] == 0


@pytest.mark.parametrize("name", sorted(R.directed_cases()))
def test_directed_cases(name):
    frames, C, params, _ties = R.directed_cases()[name]
    for period in PERIODS:
        (ap, res, ref), _ = _run(frames, C, params, None, period)
    if name == "strict":          # IoU exactly 0.5: a TP of bev@0.3; boxes one metre apart along x and otherwise equal
        _, rows = _ordered(ap)
        assert rows.tolist() == [[1 << 32, 0, 0, 0]] and res["ATE/1"] == 1.0 and res["tp_points/1"] == 40.0
    if name == "all_background":
        assert res["tp_points/1"] == 0.0 and np.isnan(res["ATE/1"]) and np.isnan(res["mATE"])


def _three_class_frames():
    """C = 4.  Class 1: two TPs and one FP.  Class 2: ground truth and detections that never meet (no TP).  Class 3: detections
    and no ground truth (npos = 0)."""
    box = R._box
    f0 = R.hand_sample([(1, 0.9, box(10, 0, 0.5, s=0.1, c=0.9)), (1, 0.7, box(40, 2)), (2, 0.8, box(20, 0)), (3, 0.6, box(30, 0)),
                        (3, 0.5, box(50, 1))], [(1, box(10.3, 0.2)), (2, box(60, 0)), (1, box(25, -3))], 4)
    f1 = R.hand_sample([(1, 0.85, box(15, 1, l=3.0)), (2, 0.4, box(35, 0))], [(1, box(15.2, 1.1, 0.25)), (2, box(5, 3))], 4)
    return [(3, f0), (7, f1)]      # (a gap in the frame indices: two updates, the frames differ in their query count)


def test_a_class_without_tps_and_a_class_without_ground_truth_are_nan():
    frames, params = _three_class_frames(), dict(R.K6, recall_points=40)
    (ap, res, ref), _ = _run(frames, 4, params, ("bev", 0.3), "2pi")
    assert ref["flags"].sum() == 2 and res["npos"].tolist() == [3.0, 2.0, 0.0]
    assert res["tp_points"].tolist() == [26.0, 0.0, 0.0]                    # recall 2 / 3: points 1..26 of 40
    assert all(np.isnan(res[f"{e}/{c}"]) for e in T.NAMES for c in (2, 3)) and not any(np.isnan(res[f"{e}/1"]) for e in T.NAMES)
    assert all(res[f"m{e}"] == res[f"{e}/1"] for e in T.NAMES)              # the mean leaves the NaN classes out


def test_a_saturating_pair_is_reported_and_gives_nan_not_a_number():
    frames, params = [(0, T.saturating_frame())], dict(R.K6, recall_points=40, roi=None)
    ref = T.run(frames, 2, min_recall=0, **params)
    assert ref["saturated"] == 1 and ref["flags"].tolist() == [True, True]
    ap = _new(2, params, tp_errors={"min_recall": 0})
    _feed(ap, frames)
    _, rows = _check_rows(ap, ref)
    assert rows[0, 0] == 1 << 52 and int(ap.state()["counters"][3]) == 1
    res = ap.compute()
    assert res["tp_saturated"] == 1.0 and torch.isnan(res["tp_err"]).all() and res["tp_points"].tolist() == [40.0]
    assert all(np.isnan(res[f"{e}/1"]) and np.isnan(res[f"m{e}"]) for e in T.NAMES)
    # the counter survives a merge, and the merged table stays NaN
    other = _new(2, params, tp_errors={"min_recall": 0})
    _feed(other, [(5, R.strict_sample())])
    other.merge(ap)
    assert other.compute()["tp_saturated"] == 1.0 and np.isnan(other.compute()["ATE/1"])


def _stream_batches(sizes):
    frames, C, params, _ = R.stream_case()
    assert sum(sizes) == len(frames)
    out, i = [], 0
    for s in sizes:
        out.append(frames[i:i + s])
        i += s
    return out, frames, C, params


TP = {"at": ["3d", 0.3], "min_recall": 0.1, "angle_period": "2pi"}


def _equal(a, b):
    (ca, ra), (cb, rb) = _ordered(a), _ordered(b)
    x, y = a.compute(), b.compute()
    return np.array_equal(ca, cb) and np.array_equal(ra, rb) and set(x) == set(y) and \
        all((x[k] == y[k]) if isinstance(x[k], list) else _same_bits(x[k], y[k]) for k in x)


def test_seven_growing_updates_merge_and_order_do_not_move_a_bit():
    batches, frames, C, params = _stream_batches([1, 3, 2, 1, 4, 2, 3])
    (whole, res, ref), = _run(frames, C, params, ("3d", 0.3), "2pi", min_recalls=(0.1,))
    assert whole.capacity == 1 << 16 and res["tp_points"].sum() > 0
    # seven updates of unequal size from a store of 64 records: both stores double five times
    ap = _new(C, params, tp_errors=TP, initial_capacity=64)
    caps = []
    for b in batches:
        _feed(ap, b)
        caps.append((ap.capacity, int(ap._tp_rows.shape[0])))
    assert caps[0] == (128, 128) and caps[-1] == (2048, 2048) and len(set(caps)) >= 3, caps
    assert _equal(ap, whole)
    # merge of two halves, and the updates in another order
    a, b = _new(C, params, tp_errors=TP, initial_capacity=64), _new(C, params, tp_errors=TP)
    for x in batches[:3]:
        _feed(a, x)
    for x in batches[3:]:
        _feed(b, x)
    a.merge(b)
    assert _equal(a, whole)
    c = _new(C, params, tp_errors=TP, initial_capacity=256)
    for x in (batches[4], batches[0], batches[6], batches[2], batches[1], batches[5], batches[3]):
        _feed(c, x)
    assert _equal(c, whole)
    # state() / load_state(), merging into an empty accumulator, reset()
    d, e = _new(C, params, tp_errors=TP), _new(C, params, tp_errors=TP)
    d.load_state(c.state())
    e.merge(d)
    assert _equal(d, whole) and _equal(e, whole)
    with pytest.raises(ValueError, match="tp_errors"):
        d.load_state({k: v for k, v in c.state().items() if k != "tp_errors"})
    c.reset()
    assert c.capacity == 0 and c._tp_rows is None and c.state()["tp_errors"].shape == (0, 4)
    _feed(c, batches[4])
    ref4 = T.run(batches[4], C, at=("3d", 0.3), min_recall=0.1, **params)
    _check_rows(c, ref4)
    assert _same_bits(c.compute()["tp_err"][:, 1:3].contiguous(), ref4["tp_err"][:, 1:3].copy())


@pytest.mark.parametrize("groups", [None, True])
def test_update_does_not_make_the_host_wait(groups):
    frames, descriptions, C, params, ref = G.stream_case()
    sizes, batches, i = [1, 3, 2, 1, 4, 2, 3, 5, 1, 6, 4], [], 0
    for s in sizes:
        batches.append(list(range(i, i + s)))
        i += s
    kw = {} if groups is None else {"groups": True, "initial_frame_capacity": 1}
    ap = _new(C, params, tp_errors=TP, initial_capacity=64, **kw)
    fed = [_batch([frames[p][1] for p in b], None if groups is None else [descriptions[p] for p in b]) for b in batches]
    torch.cuda.synchronize()
    try:
        for i, (b, (out, labels)) in enumerate(zip(batches, fed)):
            if i == 2:
                torch.cuda.set_sync_debug_mode("error")
            ap.update(out, labels, frames[b[0]][0])             # (grows the stores on the way)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _check_rows(ap, T.run(frames, C, at=("3d", 0.3), min_recall=0.1, **params))


@pytest.mark.parametrize("period", PERIODS)
def test_every_group_equals_the_restatement_and_its_ungrouped_twin(period):
    """The groups stream case: 32 frames whose time of day flips with every frame, 522 records in one class (membership flips
    inside every wave and the scan crosses two trip boundaries), groups without a frame and classes without ground truth."""
    frames, descriptions, C, params, gref = G.stream_case()
    assert G.conditions(frames, descriptions, C, params, gref) == []
    spec = {"at": ["bev", 0.5], "min_recall": 0.1, "angle_period": period}
    ap = _new(C, params, groups=True, tp_errors=spec)
    _feed(ap, frames, descriptions)
    # the whole split: rows, the "all" table and everything a grouped accumulator without the key gives
    ref = T.run(frames, C, at=("bev", 0.5), min_recall=0.1, angle_period=period, **params)
    assert np.bincount(ref["classes"]).max() > 512
    cols, rows = _check_rows(ap, ref)
    plain = _new(C, params, groups=True)
    _feed(plain, frames, descriptions)
    res = _check_plain(ap, plain)
    first = T.i_min(0.1, ap.recall_points)
    assert res["group_names"] == gref["names"] and res["tp_saturated"] == 0.0
    assert _same_bits(res["group_tp_err"][0], res["tp_err"]) and _same_bits(res["group_tp_points"][0], res["tp_points"])
    # the ungrouped entries on the same frames give the "all" table bit for bit
    flat = _new(C, params, tp_errors=spec)
    _feed(flat, frames)
    assert _same_bits(flat.compute()["tp_err"], res["tp_err"]) and _same_bits(flat.compute()["tp_points"], res["tp_points"])
    frame_of = {f: i for i, (f, _) in enumerate(frames)}
    for g, name in enumerate(gref["names"]):
        members = gref["members"][name]
        sub = [frames[i] for i in members]
        sref = T.run(sub, C, at=("bev", 0.5), min_recall=0.1, angle_period=period, **params)
        keep = np.array([frame_of[f] in set(members) for f in cols[:, 1]], dtype=bool)
        assert np.array_equal(sref["bits"], cols[keep, 4])
        _check_table(res, cols[keep], rows[keep], sref, res["group_tp_err"][g], res["group_tp_points"][g], sref["npos"],
                     ap.recall_points, first, "" if g == 0 else "/" + name)
        twin = _new(C, params, tp_errors=spec)
        _feed(twin, frames, only=members)
        t = twin.compute()
        assert _same_bits(res["group_tp_err"][g], t["tp_err"]) and _same_bits(res["group_tp_points"][g], t["tp_points"]), name


# ------------------------------------------------------------------------------------------------- the public interface
class _Stub(torch.nn.Module):
    """A 'model' that returns precomputed head outputs: data['idx'] selects the frames of the batch."""

    def __init__(self, frames):
        super().__init__()
        self.out, _ = _batch([s for _, s in frames])
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward(self, data):
        return {k: v[data["idx"]] for k, v in self.out.items()}


class _StubLoss(torch.nn.Module):
    def forward(self, output, labels):
        loss = (output["center"] ** 2).mean()
        return loss, {"center": loss}


def _loader(frames, descriptions, bs):
    batches = []
    for i in range(0, len(frames), bs):
        chunk = frames[i:i + bs]
        _, labels = _batch([s for _, s in chunk], descriptions[i:i + bs])
        batches.append(({"idx": torch.arange(i, i + len(chunk))}, labels))
    return batches


class _Writer:
    def __init__(self):
        self.tags = {}

    def add_scalar(self, tag, value, step):
        self.tags[tag] = (value, step)


def _record_calls(monkeypatch):
    from dpft_amd.hip.lib import lib
    calls, real = [], lib.call

    def call(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(lib, "call", call)
    return calls


def _tp_keys(C, tail=""):
    return {f"{e}/{c}{tail}" for e in T.NAMES for c in range(1, C)} | {f"m{e}{tail}" for e in T.NAMES} | \
        {f"tp_points/{c}{tail}" for c in range(1, C)}


@pytest.mark.parametrize("groups", [None, ["time"]])
def test_evaluate_one_epoch_returns_and_logs_the_errors_with_no_change_to_the_loop(monkeypatch, groups):
    from dpft_amd.configs import load_config
    from dpft_amd.evaluation import DataParallelEvaluator
    frames, descriptions, C, params, _ = G.stream_case()
    cfg = copy.deepcopy(load_config("kradar"))
    cfg["model"]["head"]["num_classes"] = C
    cfg["computing"] = dict(cfg.get("computing", {}), device=DEV)
    spec = {"iou": [0.3, 0.5, 0.7], "recall_points": 40, **({} if groups is None else {"groups": groups})}

    def run(spec):
        cfg["evaluate"]["dataset_ap"] = spec
        ev = DataParallelEvaluator.from_config(cfg)
        ev.eval_fn, ev.export_fn, ev.logging = None, None, "epoch"
        calls, w = _record_calls(monkeypatch), _Writer()
        got = ev.evaluate_one_epoch(2, _Stub(frames).to(DEV), _loader(frames, descriptions, 3), w, None, shard_start=frames[0][0])
        monkeypatch.undo()
        return got, w, [c for c in calls if "dataset_ap" in c]
    before, _, _ = run(spec)
    got, w, mine = run(dict(spec, tp_errors={"min_recall": 0.1}))
    new = _tp_keys(C) | {"tp_saturated"} | (set() if groups is None else _tp_keys(C, "/time=day") | _tp_keys(C, "/time=night"))
    assert set(got) == set(before) | new and set(w.tags) == {f"test/{k}" for k in got}
    assert all(_same_bits(got[k], v) for k, v in before.items())
    g = "" if groups is None else "groups_"
    assert mine == [f"dpft_dataset_ap_update_{g}tp_f32"] * 11 + [f"dpft_dataset_ap_finalize_{g}f64", f"dpft_dataset_ap_finalize_tp_{g}f64"]
    ref = T.run(frames, C, min_recall=0.1, **params)
    assert _close([got[f"{e}/{c}"] for c in range(1, C) for e in T.NAMES], ref["tp_err"].reshape(-1), UNIT)
    assert w.tags["test/mATE"] == (got["mATE"], 2) and got["mATE"] > 0


def test_trainer_validation_returns_and_logs_the_errors_with_no_change_to_the_loop(monkeypatch):
    from dpft_amd.configs import load_config
    from dpft_amd.training.trainer import DataParallelTrainer
    frames, descriptions, C, params, _ = G.stream_case()
    cfg = copy.deepcopy(load_config("kradar"))
    cfg["train"]["optimizer"] = {"name": "AdamW", "lr": 1e-2}
    cfg["model"]["head"]["num_classes"] = C
    cfg["evaluate"] = {"dataset_ap": {"iou": [0.3, 0.5, 0.7], "recall_points": 40, "tp_errors": True}}
    tr = DataParallelTrainer(_Stub(frames), cfg, torch.device(DEV))
    tr.loss_fn = _StubLoss()
    calls, w = _record_calls(monkeypatch), _Writer()
    res = tr.validate_one_epoch(1, _loader(frames, descriptions, 5), w)
    mine = [c for c in calls if "dataset_ap" in c]
    assert mine == ["dpft_dataset_ap_update_tp_f32"] * 7 + ["dpft_dataset_ap_finalize_f64", "dpft_dataset_ap_finalize_tp_f64"]
    assert _tp_keys(C) | {"tp_saturated"} <= set(res) and set(w.tags) == {f"val/{k}" for k in res}
    ref = T.run(frames, C, min_recall=0.1, **params)      # frames are numbered rank * 2^24 + local index: the same order
    assert _close([res[f"{e}/{c}"] for c in range(1, C) for e in T.NAMES], ref["tp_err"].reshape(-1), UNIT)
