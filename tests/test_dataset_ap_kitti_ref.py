"""The KITTI-protocol reference (tests/dataset_ap_kitti_ref.py) against tables worked by hand, the device path's two one-bit
reductions against the literal two passes on random small frames with many ties, and the host side of the ``kitti`` key."""
import copy

import numpy as np
import pytest

from tests import dataset_ap_kitti_ref as KR

NAN = float("nan")


def _frame(index, dets, gts, iou, num_classes):
    """A prepared frame straight from numbers: dets = [(query, class, score)], gts = [(target, class)], iou = {(query, target):
    IoU} (both kinds alike; pairs left out are 0)."""
    npos = [0] * num_classes
    for _, c in gts:
        npos[c] += 1
    full = {(n, j): (iou.get((n, j), 0.0),) * 2 for n, c, _ in dets for j, gc in gts if gc == c}
    return {"frame": index, "dets": sorted(dets), "gts": sorted(gts), "iou": full, "npos": npos, "dropped": 0}


COMBO = [("bev", 0.5)]


def _row(values):
    return list(values) + [0.0] * (KR.POINTS - len(values))


def test_hand_table_two_clean_matches():
    """Two targets, two detections, one each.  Thresholds 0.9 and 0.8, precision 1 at both, zero from the third point on:
    AP (R40) = env[1] / 40, AP11 = env[0] / 11."""
    fr = _frame(0, [(0, 1, 0.9), (1, 1, 0.8)], [(0, 1), (1, 1)], {(0, 0): 0.7, (1, 1): 0.6}, 2)
    out = KR.literal([fr], 2, COMBO)
    assert out["nthr"][0, 0] == 2 and out["thresholds"][0, 0, :2].tolist() == [0.9, 0.8] and np.isnan(out["thresholds"][0, 0, 2:]).all()
    assert out["tp"][0, 0].tolist() == _row([1, 2]) and out["fp"][0, 0].tolist() == _row([0, 0]) and out["fn"][0, 0, :2].tolist() == [1, 0]
    assert out["prec"][0, 0].tolist() == _row([1, 1]) and out["rec"][0, 0].tolist() == _row([0.5, 1])
    assert out["ap"][0, 0] == 1 / 40 and out["ap11"][0, 0] == 1 / 11 and out["mAP"] == [1 / 40]
    assert out["records"][:, 4].tolist() == [1, 1]


def test_hand_table_pass_two_rematches_what_pass_one_could_not():
    """a (0.9) overlaps t0 by 0.6 and t1 by 0.7, b (0.8) overlaps t0 by 0.8, c (0.7) overlaps t2 by 0.9.  Pass 1 (highest score):
    t0 takes a, t1 finds nothing, t2 takes c -> TP scores 0.9, 0.7, both thresholds (G = 3: i = 0 is taken at cur = 0, i = 1 is
    the last).  Pass 2 (largest IoU) at 0.9: only a is active, t0 takes it.  At 0.7: t0 takes b, t1 takes a, t2 takes c."""
    fr = _frame(4, [(0, 1, 0.9), (1, 1, 0.8), (2, 1, 0.7)], [(0, 1), (1, 1), (2, 1)],
                {(0, 0): 0.6, (0, 1): 0.7, (1, 0): 0.8, (2, 2): 0.9}, 2)
    out = KR.literal([fr], 2, COMBO)
    assert out["thresholds"][0, 0, :2].tolist() == [0.9, 0.7] and out["nthr"][0, 0] == 2
    assert out["tp"][0, 0].tolist() == _row([1, 3]) and out["fp"][0, 0].tolist() == _row([0, 0])
    assert out["rec"][0, 0].tolist() == _row([1 / 3, 1.0]) and out["prec"][0, 0].tolist() == _row([1, 1])
    assert out["records"][:, 4].tolist() == [1, 0, 1]                      # by score: a and c are pass-1 TPs, b is not
    assert out["tiesums"][(4, 1, 0.9)] == [1] and out["tiesums"][(4, 1, 0.8)] == [2] and out["tiesums"][(4, 1, 0.7)] == [3]
    bits = KR.frame_bits(fr, 1, 0, 0.5)
    assert bits == {0: (1, 1), 1: (0, 1), 2: (1, 1)}                       # inserting b displaces a from t0 on to t1


def test_hand_table_false_positive_empty_class_and_class_without_tp():
    """Class 1: x (0.9) overlaps nothing, y (0.5) matches the only target: one threshold 0.5 with TP 1, FP 1.  Class 2 has a
    target and no detection: 0.  Class 3 has a detection and no target: NaN, and stays out of the mean."""
    fr = _frame(0, [(0, 1, 0.9), (1, 1, 0.5), (2, 3, 0.8)], [(0, 1), (1, 2)], {(1, 0): 0.8}, 4)
    out = KR.literal([fr], 4, COMBO)
    assert out["nthr"][:, 0].tolist() == [1, 0, 0] and out["thresholds"][0, 0, 0] == 0.5
    assert out["tp"][0, 0, 0] == 1 and out["fp"][0, 0, 0] == 1 and out["prec"][0, 0, 0] == 0.5 and out["rec"][0, 0, 0] == 1
    assert out["ap"][:2, 0].tolist() == [0.0, 0.0] and np.isnan(out["ap"][2, 0])
    assert out["ap11"][0, 0] == 0.5 / 11 and out["ap11"][1, 0] == 0.0 and np.isnan(out["ap11"][2, 0])
    assert out["mAP"] == [0.0] and out["mAP11"] == [0.5 / 11 / 2]


def test_hand_negative_scores_take_no_part_in_pass_one():
    """min_score < 0 lets negative scores in: pass 1 (score threshold 0.0) passes them over, pass 2 never sees them because every
    threshold is a pass-1 TP score."""
    fr = _frame(0, [(0, 1, -0.5), (1, 1, 0.25)], [(0, 1), (1, 1)], {(0, 0): 0.9, (1, 1): 0.9}, 2)
    out = KR.literal([fr], 2, COMBO)
    assert out["thresholds"][0, 0, 0] == 0.25 and out["nthr"][0, 0] == 1 and out["tp"][0, 0, 0] == 1 and out["fp"][0, 0, 0] == 0
    assert out["records"][:, 4].tolist() == [1, 0]


def test_threshold_loop_sample_counts():
    """41 sample points: n1 = G = 100 picks 41 scores, the first and the last among them; recall steps wider than 1 / 40 take every
    score, narrower ones skip ranks, and the last rank is never skipped."""
    scores = [1.0 - i / 1000 for i in range(100)]
    got = KR.pick_thresholds(scores, 100)
    assert len(got) == 41 and got[0] == scores[0] and got[-1] == scores[-1] and got == sorted(got, reverse=True)
    assert KR.pick_thresholds(scores[:7], 7) == scores[:7] and KR.pick_thresholds([], 5) == []      # recall steps of 1/7 > 1/40
    assert KR.pick_thresholds(scores[:3], 1000) == [scores[0], scores[2]]      # recall 0.002 is skipped, the last rank never is
    assert len(KR.pick_thresholds(scores[:41], 41)) == 41 and len(KR.pick_thresholds(scores[:40], 40)) == 40
    for G in (1000, 12345):
        assert len(KR.pick_thresholds([1.0 - i / 20000 for i in range(G)], G)) == 41


def test_the_kernels_rank_selection_equals_the_literal_loop_on_the_host():
    """csrc/ap_kitti.h jumps over the skipped ranks instead of visiting them; ``dpft_dataset_ap_kitti_ranks`` is that function on
    the host.  Its ranks must be the literal loop's for every n1 <= G up to 160, for n1 = G and random n1 up to G = 1500 and a few
    G up to 2 * 10^5, and the run must meet (r - cur) == (cur - l) exactly many times, which is where a predicate that is only
    approximately right would slip."""
    import ctypes as C
    from dpft_amd.hip.lib import lib
    dll = lib.load()
    out = (C.c_int64 * KR.POINTS)()
    rng = np.random.default_rng(41)
    pairs = [(n1, G) for G in range(1, 161) for n1 in range(G + 1)]
    pairs += [(G, G) for G in range(161, 1500, 3)] + [(int(rng.integers(1, G + 1)), G) for G in range(162, 1500, 3)]
    pairs += [(int(rng.integers(G // 2, G + 1)), G) for G in rng.integers(10 ** 4, 2 * 10 ** 5, 12).tolist()]
    exact = {}
    for n1, G in pairs:
        want = KR.pick_thresholds(list(range(n1)), G, exact if G < 1500 else None)      # "scores" = their own ranks
        nt = dll.dpft_dataset_ap_kitti_ranks(n1, G, out)
        assert nt == len(want) <= KR.POINTS and list(out[:nt]) == want, (n1, G)
    assert exact["exact"] > 1000
    assert dll.dpft_dataset_ap_kitti_ranks(3, 2, out) < 0 and dll.dpft_dataset_ap_kitti_ranks(0, 0, out) < 0
    assert dll.dpft_dataset_ap_kitti_ranks(1, 1, None) < 0 and "null" in lib.dpft_last_error().decode()


def _random_frames(rng, n_frames, C):
    """D <= 9 detections, M <= 6 targets, scores and IoUs out of a few values: ties everywhere."""
    frames = []
    for f in range(n_frames):
        D, M = int(rng.integers(0, 10)), int(rng.integers(0, 7))
        dets = [(n, int(rng.integers(1, C)), float(rng.choice([-0.25, 0.0, 0.25, 0.5, 0.5, 0.75]))) for n in range(D)]
        gts = [(j, int(rng.integers(1, C))) for j in range(M)]
        iou = {(n, j): float(rng.choice([0.0, 0.0, 0.4, 0.5, 0.6, 0.6, 0.8])) for n in range(D) for j in range(M)}
        frames.append(_frame(10 + f, dets, gts, iou, C))
    return frames


@pytest.mark.parametrize("seed", range(4))
def test_reductions_equal_the_literal_form_on_random_tied_frames(seed):
    """The one-bit reductions give the thresholds, TP and FP of the literal two passes at every threshold -- and therefore the same
    precision, recall, AP and AP11 to the bit."""
    rng = np.random.default_rng(900 + seed)
    combos = [("bev", 0.5), ("3d", 0.3)]
    for _ in range(60):
        C = int(rng.integers(2, 4))
        frames = _random_frames(rng, int(rng.integers(1, 5)), C)
        lit, red = KR.literal(frames, C, combos), KR.reduced(frames, C, combos)
        for key in ("nthr", "thresholds", "tp", "fp", "fn", "prec", "rec", "ap", "ap11", "npos"):
            assert np.array_equal(lit[key], red[key], equal_nan=True), (key, lit[key], red[key])
        # the pass-1 bit itself, and the pass-2 bits summed to the end of every score tie group of a frame
        for fr in frames:
            for c in range(1, C):
                for k, (kind, thr) in enumerate(combos):
                    bits = KR.frame_bits(fr, c, 0, thr)
                    for n, dc, s in fr["dets"]:
                        if dc != c:
                            continue
                        want1 = int(((lit["records"][(lit["records"][:, 1] == fr["frame"]) & (lit["records"][:, 2] == n), 4][0]) >> k) & 1)
                        assert bits[n][0] == want1
                        upto = sum(bits[m][1] for m, mc, ms in fr["dets"] if mc == c and ms >= s)
                        assert upto == lit["tiesums"][(fr["frame"], c, s)][k]


# ------------------------------------------------------------------------------------------------------------ the host side
def _config(spec):
    from dpft_amd.configs import load_config
    cfg = copy.deepcopy(load_config("kradar"))
    cfg["evaluate"]["dataset_ap"] = spec
    return cfg


def test_config_key_is_a_bool_and_off_by_default():
    from dpft_amd.evaluation.dataset_ap import DatasetAP
    assert DatasetAP.from_config(_config(True)).kitti is False
    assert DatasetAP.from_config(_config({"kitti": False})).kitti is False
    assert DatasetAP.from_config(_config({"kitti": True, "iou": [0.5]})).kitti is True
    assert DatasetAP(3, kitti=True).kitti is True
    for bad in (1, "yes", 0.5, [True]):
        with pytest.raises(ValueError, match="kitti"):
            DatasetAP.from_config(_config({"kitti": bad}))
    with pytest.raises(ValueError, match="kitti"):                            # the list of known keys names it
        DatasetAP.from_config(_config({"kiti": True}))
    a, b = DatasetAP(2, kitti=True), DatasetAP(2)
    with pytest.raises(ValueError, match="parameters"):
        a.merge(b)


def test_key_names_with_and_without_groups_and_nothing_new_without_the_key():
    from dpft_amd.evaluation.dataset_ap import KITTI_POINTS, DatasetAP
    plain = DatasetAP(3, iou=[0.5], kinds=["3d"])
    assert not [k for k in plain.compute() if "kitti" in k]
    ap = DatasetAP(3, iou=[0.5], kinds=["3d"], kitti=True)
    res = ap.compute()                                                        # nothing accumulated: NaN table, no library call
    scalars = {"kitti/AP_3d@0.5/1", "kitti/AP_3d@0.5/2", "kitti/AP11_3d@0.5/1", "kitti/AP11_3d@0.5/2", "kitti/mAP_3d@0.5",
               "kitti/mAP11_3d@0.5"}
    tensors = {"kitti_ap", "kitti_ap11", "kitti_prec", "kitti_rec", "kitti_thresholds", "kitti_tp", "kitti_fp", "kitti_nthr"}
    assert {k for k in res if "kitti" in k} == scalars | tensors
    assert set(ap.scalars()) - set(plain.scalars()) == scalars and all(v != v for k, v in ap.scalars().items() if k in scalars)
    assert res["kitti_ap"].shape == (2, 1) and res["kitti_prec"].shape == (2, 1, KITTI_POINTS) == res["kitti_thresholds"].shape
    assert res["kitti_nthr"].shape == (2, 1) and int(res["kitti_nthr"].sum()) == 0 and bool(res["kitti_thresholds"].isnan().all())
    grouped = DatasetAP(3, iou=[0.5], kinds=["3d"], kitti=True, groups=["time"], tp_errors=True)
    res = grouped.compute()
    names = grouped.group_names
    assert names == ["all", "time=day", "time=night"]
    want = scalars | {f"{k}/{g}" for k in scalars for g in names[1:]}
    assert {k for k, v in res.items() if k.startswith("kitti/")} == want
    assert res["group_kitti_ap"].shape == (3, 2, 1) == res["group_kitti_ap11"].shape and res["kitti_ap"].shape == (2, 1)
    assert {k for k in grouped.scalars() if k.startswith("kitti/")} == want
