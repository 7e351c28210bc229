"""The fp64 restatement of the split-level AP (tests/dataset_ap_ref.py) against hand-checked values, and the builder's promise
that every case the GPU tests compare on is safe to compare bit for bit.  No GPU."""
import math

import numpy as np
import pytest

from tests import dataset_ap_ref as R


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_shape_cases_keep_the_three_conditions(name):
    frames, C, params, ref = R.shape_case(name)
    assert R.violations(frames, C, params) == []
    N, ms, C0, _ = R.SHAPES[name]
    assert C == C0 and [f[1]["cls"].shape for f in frames] == [(N, C)] * len(ms)
    assert [f[1]["gt_class"].shape[0] for f in frames] == ms
    if N >= 63:      # a case that never matched anything would test nothing
        assert ref["tp"].sum() > 0 and len(ref["records"]) > N // 4


def test_stream_and_directed_cases_keep_the_three_conditions():
    frames, C, params, ref = R.stream_case()
    assert R.violations(frames, C, params) == [] and ref["tp"].sum() > 0
    for name, (frames, C, params, ties) in R.directed_cases().items():
        if name == "strict":      # an IoU exactly ON a threshold is that case's point (both sides are exact there: below)
            continue
        assert R.violations(frames, C, params, ties_allowed=ties) == [], name


def _one_class(flags, npos, Rn=40):
    """records of class 1 with the given TP flags (already in order)"""
    recs = [[1.0 - 0.01 * i, 0, i, 1, int(f)] for i, f in enumerate(flags)]
    return R.average_precision(recs, npos, 0, Rn)


def test_hand_checked_average_precisions():
    # two targets, records TP FP TP: recall 0.5 from position 0 (precision 1), recall 1 at position 2 (precision 2/3)
    ap, tp = _one_class([1, 0, 1], 2)
    assert tp == 2 and abs(ap - (20 * 1.0 + 20 * (2 / 3)) / 40) <= 1e-12      # (40 fp64 terms summed one by one)
    # no detection at all: every envelope value is 0
    assert _one_class([], 3) == (0.0, 0)
    # no ground truth: NaN, and the class is left out of the mean
    ap, _ = _one_class([0, 0], 0)
    assert math.isnan(ap)
    box = R._box(10, 0)
    frames = [(0, R.hand_sample([(1, 0.9, box), (1, 0.8, box), (2, 0.7, R._box(30, 0))], [(1, box)], 3))]
    res = R.run(frames, 3, kinds=("3d",), iou=(0.5,))
    # duplicates on one target: the second is an FP
    assert res["records"][:, 4].tolist() == [1, 0, 0] and res["records"][:, 2].tolist() == [0, 1, 2]
    assert res["npos"].tolist() == [1.0, 0.0] and res["ap"][0, 0] == 1.0 and math.isnan(res["ap"][1, 0])
    assert res["mAP"] == [1.0]                                  # class 2 (npos 0) excluded
    none = R.run([(0, R.hand_sample([], [], 3))], 3)
    assert all(math.isnan(v) for v in none["mAP"]) and none["records"].shape == (0, 5)


def test_strictly_greater_than_the_threshold_on_exact_geometry():
    s = R.strict_sample()
    bev, d3 = R.iou_pair(s["center"][0], s["size"][0], s["angle"][0], s["gt_center"][0], s["gt_size"][0], s["gt_angle"][0])
    assert bev == 0.5 and d3 == 0.5                              # exactly
    res = R.run([(0, s)], 2, kinds=("bev", "3d"), iou=(0.3, 0.5))
    # combinations: bev@0.3, bev@0.5, 3d@0.3, 3d@0.5 -> matched at 0.3 only
    assert res["records"][0, 4] == 0b0101
    assert res["ap"][0].tolist() == [1.0, 0.0, 1.0, 0.0]


def test_reference_details():
    # argmax: first maximum, a NaN counts as the maximum; score filter in fp32 with >=; roi strict
    assert R.in_roi((0.5, 0, 0), R.DEFAULT_ROI) and not R.in_roi((0.0, 0, 0), R.DEFAULT_ROI)
    assert not R.in_roi((10, np.float32(6.4), 0), R.DEFAULT_ROI) and R.in_roi((10, 100, 0), None)
    cases = R.directed_cases()
    frames, C, params, _ = cases["min_score_equal"]
    res = R.run(frames, C, **params)
    assert sorted(res["records"][:, 2].tolist()) == [0, 2]       # the score equal to min_score stays, the next lower float goes
    frames, C, params, _ = cases["nan_score"]
    res = R.run(frames, C, **params)
    assert res["dropped_nan"] == 2 and res["records"][:, 2].tolist() == [1]
    frames, C, params, _ = cases["roi_faces"]
    res = R.run(frames, C, **params)
    assert sorted(res["records"][:, 2].tolist()) == [12, 13, 14, 15, 16, 17]
    frames, C, params, _ = cases["roi_null"]
    assert len(R.run(frames, C, **params)["records"]) == 18
    frames, C, params, _ = cases["five_for_one"]
    assert R.run(frames, C, **params)["tp"][0].max() == 1.0
    # invalid boxes have IoU 0 with anything
    assert R.iou_pair((0, 0, 0), (2, 2, 2), (0, 0), (0, 0, 0), (2, 2, 2), (0, 1)) == (0.0, 0.0)
    assert R.iou_pair((0, 0, 0), (2, 2, 0), (0, 1), (0, 0, 0), (2, 2, 2), (0, 1)) == (0.0, 0.0)
    b, d = R.iou_pair((0, 0, 0), (2, 2, 2), (0, 3), (0, 0, 0), (2, 2, 2), (0, 1))      # (sin, cos) is normalised
    assert b == 1.0 and d == 1.0
