"""The restatement of the true-positive errors (tests/dataset_ap_tp_ref.py) on cases whose answers are known in closed form, and
its TP flags against tests/dataset_ap_ref.py's bits on every shape case.  No GPU."""
import math

import numpy as np
import pytest

from tests import dataset_ap_ref as R
from tests import dataset_ap_tp_ref as T

F32 = np.float32
ONE = 1 << 32


def _b(x=10.0, y=0.0, z=0.0, l=4.0, w=2.0, h=1.5, s=0.0, c=1.0):
    a = np.array([x, y, z, l, w, h, s, c], dtype=F32)
    return a[:3], a[3:6], a[6:]


def _err(d, g, period="2pi"):
    return T.errors(*d, *g, period)


def test_closed_form_errors_and_their_integers():
    ate, aze, ase, aoe = _err(_b(13, 4, 0), _b(10, 0, 0))                  # shifted by (3, 4, 0)
    assert (ate, aze, ase, aoe) == (5.0, 0.0, 0.0, 0.0) and T.quantise(ate) == (5 * ONE, False)
    assert _err(_b(z=0.25), _b())[1] == 0.25 and T.quantise(0.25) == (ONE // 4, False)
    assert _err(_b(s=0.6, c=0.8), _b(s=0.6, c=0.8)) == (0.0, 0.0, 0.0, 0.0)
    assert _err(_b(l=2.0), _b(l=4.0))[2] == 0.5 and _err(_b(l=4.0), _b(l=2.0))[2] == 0.5      # half the length, either way
    assert _err(_b(s=1.0, c=0.0), _b())[3] == math.pi / 2                  # a quarter turn
    assert _err(_b(s=-1.0, c=0.0), _b())[3] == math.pi / 2                 # the sign of the turn does not matter
    assert _err(_b(s=0.0, c=-1.0), _b())[3] == math.pi and _err(_b(s=0.0, c=-1.0), _b(), "pi")[3] == 0.0
    s = math.sin(3 * math.pi / 4)
    a2, api = _err(_b(s=s, c=-s), _b())[3], _err(_b(s=s, c=-s), _b(), "pi")[3]
    assert abs(a2 - 3 * math.pi / 4) < 1e-7 and abs(api - math.pi / 4) < 1e-7 and api == math.pi - a2      # fp32 inputs


def test_unnormalised_angle_pairs_give_the_same_error():
    yaw_d, yaw_g = 0.7, -0.4
    want = _err(_b(s=math.sin(yaw_d), c=math.cos(yaw_d)), _b(s=math.sin(yaw_g), c=math.cos(yaw_g)))[3]
    assert abs(want - 1.1) < 1e-6
    for scale_d, scale_g in ((0.5, 1.0), (2.0, 0.25), (1.75, 1.75)):
        got = _err(_b(s=scale_d * math.sin(yaw_d), c=scale_d * math.cos(yaw_d)),
                   _b(s=scale_g * math.sin(yaw_g), c=scale_g * math.cos(yaw_g)))[3]
        assert abs(got - want) < 1e-6, (scale_d, scale_g)                  # (the fp32 rounding of the scaled pair)
    assert _err(_b(s=1.5, c=0.0), _b(s=0.0, c=0.25))[3] == math.pi / 2     # exact pairs: exactly the same


def test_quantise_rounds_half_to_even_and_saturates():
    assert T.quantise(0.5 / ONE) == (0, False) and T.quantise(1.5 / ONE) == (2, False) and T.quantise(2.5 / ONE) == (2, False)
    assert T.quantise(-1.5 / ONE) == (-2, False)
    below = float(np.nextafter(T.LIMIT, 0.0))
    # (2^52 - 0.5 rounds to the even 2^52: the counter says what saturated, not the stored value)
    assert T.quantise(below) == (T.SATURATED, False) and below * ONE == T.SATURATED - 0.5
    for bad in (T.LIMIT, 2.0e6, float("inf"), float("nan"), -T.LIMIT):
        assert T.quantise(bad) == (T.SATURATED, True)


def _points(npos, R_, flags, first=1):
    """Served points per TP count and the class result, with error rows = (T, 2T, 0, 0) * 2^32 for the T-th TP."""
    rows, t = [], 0
    for f in flags:
        t += f
        rows.append([t * ONE, 2 * t * ONE, 0, 0] if f else [0, 0, 0, 0])
    return T.class_errors(flags, rows, npos, R_, first)


def test_point_rule_below_at_and_above_the_number_of_points():
    # npos < R: one TP serves several points.  npos = 2, R = 4: TP 1 serves 1..2 (mean 1), TP 2 serves 3..4 (mean 1.5)
    err, n = _points(2, 4, [1, 0, 1])
    assert n == 4 and err[0] == (1 + 1 + 1.5 + 1.5) / 4 and err[1] == 2 * err[0] and err[2:] == [0.0, 0.0]
    # npos = 1: the one TP serves every point
    assert _points(1, 5, [0, 1]) == ([1.0, 2.0, 0.0, 0.0], 5)
    # npos = R: the T-th TP serves point T alone; cumulative means 1, 1.5, 2 -- and the unmatched fourth target leaves point 4 out
    err, n = _points(4, 4, [1, 1, 0, 1])
    assert n == 3 and err[0] == (1 + 1.5 + 2) / 3
    # npos > R: TPs that serve no point.  npos = 5, R = 2: TP 1, 2 none (floor(2 * 2 / 5) = 0), TP 3 point 1, TP 4 none, TP 5 point 2
    err, n = _points(5, 2, [1, 1, 1, 1, 1])
    assert n == 2 and err[0] == ((1 + 2 + 3) / 3 + (1 + 2 + 3 + 4 + 5) / 5) / 2
    err, n = _points(5, 2, [1, 1, 0, 0])
    assert n == 0 and all(math.isnan(v) for v in err)                      # recall 2 / 5 reaches no point
    # no TP at all, and no ground truth
    assert _points(3, 4, [0, 0])[1] == 0 and math.isnan(_points(3, 4, [0, 0])[0][0])
    assert _points(0, 4, [0, 0])[1] == 0 and math.isnan(_points(0, 4, [])[0][3])


def test_min_recall_is_exact_and_cuts_the_low_points():
    assert [T.i_min(m, 40) for m in (0, 0.0, 0.1, 0.3, 0.7, 1, 1.0)] == [1, 1, 4, 12, 28, 40, 40]
    assert T.i_min(0.1, 101) == 11 and T.i_min(0.1, 10) == 1 and T.i_min(0.01, 2) == 1 and T.i_min(0.29, 100) == 29
    flags = [1] * 10                                                        # npos = 10, R = 40: TP T serves 4T-3 .. 4T
    means = [(t + 1) / 2 for t in range(1, 11)]
    all_pts, n = _points(10, 40, flags, T.i_min(0, 40))
    assert n == 40 and all_pts[0] == sum(m for m in means for _ in range(4)) / 40
    cut, n = _points(10, 40, flags, T.i_min(0.1, 40))                       # points 4..40: one of TP 1's four is left
    assert n == 37 and cut[0] == sum([means[0]] + [m for m in means[1:] for _ in range(4)]) / 37
    last, n = _points(10, 40, flags, T.i_min(1, 40))                        # point 40 alone
    assert n == 1 and last[0] == means[-1]
    # best recall 3 / 10 below min_recall 0.5: NaN, not the mean of nothing
    err, n = _points(10, 40, [1, 1, 1, 0], T.i_min(0.5, 40))
    assert n == 0 and all(math.isnan(v) for v in err)
    assert _points(10, 40, [1, 1, 1, 0], T.i_min(0.3, 40))[1] == 1          # recall 0.3 reaches point 12 exactly


def test_run_on_a_hand_frame():
    box = R._box
    sample = R.hand_sample([(1, 0.9, box(13, 4, 0.25)), (1, 0.8, box(30, 0, l=2.0)), (1, 0.7, box(50, 0)), (2, 0.6, box(20, 0))],
                           [(1, box(13.3, 4.4)), (1, box(30, 0)), (2, box(60, 0))], 3)
    ref = T.run([(0, sample)], 3, at=("bev", 0.3), min_recall=0, recall_points=4)
    assert ref["flags"].tolist() == [True, True, False, False] and ref["k"] == 0 and ref["saturated"] == 0
    d = math.sqrt((13.0 - float(F32(13.3))) ** 2 + (4.0 - float(F32(4.4))) ** 2)
    assert ref["rows"][0].tolist() == [round(d * ONE), ONE // 4, 0, 0] and ref["rows"][1].tolist() == [0, 0, ONE // 2, 0]
    assert ref["rows"][2:].tolist() == [[0] * 4] * 2
    # class 1: npos 2, R 4: points 1..2 hold TP 1's errors, 3..4 the means of both; class 2: no TP
    a, b = round(d * ONE) / ONE, round(d * ONE) / ONE / 2
    assert ref["tp_err"][0].tolist() == [(((a + a) + b) + b) / 4, (0.25 + 0.25 + 0.125 + 0.125) / 4, (0.0 + 0.0 + 0.25 + 0.25) / 4, 0.0]
    assert ref["tp_points"].tolist() == [4.0, 0.0] and np.isnan(ref["tp_err"][1]).all()
    assert ref["mean"] == ref["tp_err"][0].tolist()                         # the NaN class is left out of the mean


def test_saturation_is_counted():
    ref = T.run([(0, T.saturating_frame())], 2, min_recall=0, roi=None)
    assert ref["flags"].tolist() == [True, True] and ref["saturated"] == 1
    assert ref["rows"][0].tolist() == [T.SATURATED, ONE // 2, 0, 0] and ref["rows"][1, 0] < ONE


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_tp_flags_equal_the_ap_references_bits_on_every_shape(name):
    frames, C, params, ref = R.shape_case(name)
    combos = R.combinations(params["kinds"], params["iou"])
    roi = params.get("roi", R.DEFAULT_ROI)
    ks = sorted({0, len(combos) // 2, len(combos) - 1})
    for f, sample in frames:
        recs, _, _ = R.frame_records(f, sample, C, combos, 0.0, roi)
        for k in ks:
            taken = T.frame_matches(sample, C, combos[k][0], combos[k][1], 0.0, roi)
            assert {n for _, _, n, _, bits in recs if (bits >> k) & 1} == set(taken), (name, f, k)
            assert len(set(taken.values())) == len(taken)                  # a target is taken once
    # and the whole restatement lines its rows up with the AP reference's records
    got = T.run(frames, C, min_recall=0, **params)
    assert np.array_equal(got["bits"], ref["records"][:, 4]) and np.array_equal(got["classes"], ref["records"][:, 3])
    assert np.array_equal(got["flags"], (ref["records"][:, 4] >> got["k"]) & 1 == 1)
    assert np.array_equal(got["rows"].any(1) <= got["flags"], np.ones(len(got["flags"]), dtype=bool))      # non-TP rows are zeros


def test_the_crowded_shape_serves_no_point_at_min_recall_0p1():
    """n65_m256_c8_k1_r40: recall stays below 0.1 in every class, so only min_recall 0 compares numbers there."""
    frames, C, params, _ = R.shape_case("n65_m256_c8_k1_r40")
    assert T.run(frames, C, min_recall=0.1, **params)["tp_points"].sum() == 0
    assert T.run(frames, C, min_recall=0, **params)["tp_points"].sum() > 0
