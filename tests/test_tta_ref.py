"""The fp64 restatement of the test-time-augmentation fusion (tests/tta_ref.py) on hand-built cases with known answers.  No GPU."""
import numpy as np

from tests import dataset_ap_ref as G
from tests import nms_ref as N
from tests import tta_ref as R

f32 = np.float32
B = G._box


def _views(*dets_per_view, C=2):
    """dets_per_view[t] = [(class, score, box)] -> views[t] = [one frame], padded to the longest view with background rows."""
    n = max(len(d) for d in dets_per_view)
    return [[N.hand_frame(d, C, n)] for d in dets_per_view]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def test_two_identical_boxes_from_two_views():
    box = B(10, 3, 0.5, 4, 2, 1.5, 0.6, 0.8)
    views = _views([(1, 0.6, box)], [(1, 0.2, box)])
    for score, want in (("mean", f32((np.float64(f32(0.6)) + np.float64(f32(0.2))) / 2)), ("max", f32(0.6))):
        out, _ = R.run(views, (False, False), score=score)
        assert out["status"].tolist() == [[-1, 0]] and out["members"].tolist() == [[2, 0]] and out["counts"].tolist() == [1]
        assert np.array_equal(out["center"][0, 0], f32(box[:3])) and np.array_equal(out["size"][0, 0], f32(box[3:6]))
        assert np.allclose(out["angle"][0, 0], box[6:], rtol=0, atol=1e-7)
        assert out["cls"][0, 0].tolist() == [0.0, want]
        assert abs(float(want) - (0.4 if score == "mean" else 0.6)) < 1e-7
        # the member keeps its geometry bits and reads as background: [0] = its score
        assert out["cls"][0, 1].tolist() == [f32(0.2), f32(0.2)]
        assert np.array_equal(_bits(out["center"][0, 1]), _bits(box[:3]))


def test_a_flipped_row_lands_on_the_box_of_view_0():
    views = _views([(1, 0.9, B(10, 3, s=0.5, c=0.8))], [(1, 0.8, B(10, -3, s=-0.5, c=0.8))])
    out, frames = R.run(views, (False, True))
    assert frames[0]["center"][1].tolist() == [10.0, 3.0, 0.0] and frames[0]["angle"][1].tolist() == [0.5, f32(0.8)]
    assert out["status"].tolist() == [[-1, 0]] and out["members"].tolist() == [[2, 0]]
    assert out["center"][0, 0].tolist() == [10.0, 3.0, 0.0]
    # unflipped the two are 6 m apart: two clusters of one, each with half its score
    out, _ = R.run(views, (False, False))
    assert out["status"].tolist() == [[-1, -1]] and out["members"].tolist() == [[1, 1]]
    assert out["cls"][0, :, 1].tolist() == [f32(np.float64(f32(0.9)) / 2), f32(np.float64(f32(0.8)) / 2)]


def test_the_sign_bit_is_flipped_not_the_value_negated():
    views = _views([(1, 0.9, B(10, 0.0))], [(1, 0.8, B(30, 0.0))])
    views[1][0]["center"][0, 1] = f32(-0.0)
    views[1][0]["angle"][0, 0] = f32("nan")
    _, frames = R.run(views, (False, True))
    assert _bits(frames[0]["center"][1, 1]) == 0 and _bits(frames[0]["center"][0, 1]) == 0
    assert _bits(frames[0]["angle"][1, 0]) == _bits(views[1][0]["angle"][0, 0]) ^ np.uint32(0x80000000)


def test_a_box_found_in_one_of_two_views_halves_its_score_under_mean():
    views = _views([(1, 0.5, B(10, 0)), (1, 0.75, B(40, 2))], [(1, 0.25, B(10.1, 0))])
    out, _ = R.run(views, (False, False), score="mean")
    assert out["members"].tolist() == [[2, 1, 0, 0]]
    assert out["cls"][0, 1].tolist() == [0.0, 0.375] and out["cls"][0, 0].tolist() == [0.0, 0.375]
    assert np.array_equal(_bits(out["center"][0, 1]), _bits([40, 2, 0]))           # a cluster of one keeps its bits
    out, _ = R.run(views, (False, False), score="max")
    assert out["cls"][0, 1].tolist() == [0.0, 0.75] and out["cls"][0, 0].tolist() == [0.0, 0.5]


def test_a_suppressed_candidate_suppresses_nothing_the_chain():
    # IoU(A, B) = 0.6, IoU(B, C) = 5 / 11, IoU(A, C) = 3 / 13 < 0.3: C heads its own cluster
    views = _views([(1, 0.9, B(10, 0)), (1, 0.7, B(12.5, 0))], [(1, 0.8, B(11, 0))])
    out, _ = R.run(views, (False, False))
    assert out["status"].tolist() == [[-1, -1, 0, -2]] and out["members"].tolist() == [[2, 1, 0, 0]]
    w = [np.float64(f32(0.9)), np.float64(f32(0.8))]
    assert out["center"][0, 0, 0] == f32((w[0] * 10.0 + w[1] * 11.0) / (w[0] + w[1]))
    assert out["center"][0, 1].tolist() == [12.5, 0.0, 0.0]
    assert out["cls"][0, 3].tolist() == [0.5, 0.0]                                  # the padding row: no candidate, untouched


def test_an_opposed_heading_is_left_out_of_the_angle_but_not_of_the_centre():
    views = _views([(1, 0.5, B(10, 0, s=0.0, c=1.0))], [(1, 0.5, B(10.5, 0, s=0.0, c=-1.0))])
    out, _ = R.run(views, (False, False))
    assert out["status"].tolist() == [[-1, 0]]
    assert out["center"][0, 0].tolist() == [10.25, 0.0, 0.0] and out["angle"][0, 0].tolist() == [0.0, 1.0]
    # at a right angle (dot = 0, not negative) the member votes: (0, 1) and (1, 0) average to (0.5, 0.5)
    views = _views([(1, 0.5, B(10, 0, l=2.0, w=2.0, s=0.0, c=1.0))], [(1, 0.5, B(10, 0, l=2.0, w=2.0, s=2.0, c=0.0))])
    out, _ = R.run(views, (False, False))
    assert out["angle"][0, 0].tolist() == [0.5, 0.5]


def test_a_cluster_of_three_in_two_views_divides_by_three():
    views = _views([(1, 0.75, B(10, 0)), (1, 0.5, B(10.1, 0))], [(1, 0.25, B(10.2, 0))])
    out, _ = R.run(views, (False, False), score="mean")
    assert out["members"].tolist() == [[3, 0, 0, 0]] and out["status"].tolist() == [[-1, 0, 0, -2]]
    assert out["cls"][0, 0].tolist() == [0.0, 0.5]
    c = (0.75 * 10.0 + 0.5 * np.float64(f32(10.1)) + 0.25 * np.float64(f32(10.2))) / 1.5
    assert out["center"][0, 0, 0] == f32(c)


def test_a_singleton_with_nan_geometry_keeps_its_bits():
    nan = float("nan")
    views = _views([(1, 0.9, B(nan, 0)), (1, 0.6, B(20, 0, s=0.0, c=0.0))], [(1, 0.8, B(10, 0, l=float("inf"))), (1, 0.7, B(20, 0))])
    before = R.union(views, (False, True))[0]
    out, _ = R.run(views, (False, True))
    assert out["status"].tolist() == [[-1, -1, -1, -1]] and out["members"].tolist() == [[1, 1, 1, 1]]
    for k in ("center", "size", "angle"):
        assert np.array_equal(_bits(out[k][0]), _bits(before[k]))
    assert out["cls"][0, :, 1].tolist() == [f32(np.float64(f32(s)) / 2) for s in (0.9, 0.6, 0.8, 0.7)]


def test_weights_of_zero_and_infinite_scores():
    inf = float("inf")
    views = _views([(1, inf, B(10, 0))], [(1, 0.5, B(10.5, 0))])
    out, _ = R.run(views, (False, False))
    assert out["center"][0, 0].tolist() == [10.5, 0.0, 0.0] and out["cls"][0, 0].tolist() == [0.0, inf]      # w(inf) = 0
    views = _views([(1, 0.0, B(10, 0))], [(1, 0.0, B(10.5, 0))])
    for v in views:
        v[0]["cls"][:, 0] = f32(-1.0)
    out, _ = R.run(views, (False, False))
    assert out["members"].tolist() == [[2, 0]] and out["center"][0, 0].tolist() == [10.0, 0.0, 0.0]           # sum w = 0


def test_below_min_score_rows_take_no_part():
    views = _views([(1, 0.9, B(10, 0))], [(1, 0.2, B(10.1, 0))])
    out, _ = R.run(views, (False, False), min_score=0.5)
    assert out["status"].tolist() == [[-1, -3]] and out["members"].tolist() == [[1, 0]]
    assert out["cls"][0, 1].tolist() == [f32(0.2), f32(0.2)] and out["center"][0, 0].tolist() == [10.0, 0.0, 0.0]


def test_the_seeded_cases_hold_what_they_promise():
    views, frames, params = R.shape_case(2, 33, 2, 3, (False, True), "bev")
    ref = R.shape_reference(2, 33, 2, 3, (False, True), "bev", "mean")
    m = ref["members"]
    assert (m[0] == 1).any() and (m[0] == 2).any() and (m > 2).any()
    n = 32
    assert ref["status"][0, n - 1] == n and ref["status"][0, 33 + n] == n and m[0, n] == 3      # two members of view 0, one of view 1
    assert ref["status"][0, 33 + n - 2] == n - 2                                                # the tie goes to the lower id
    assert _bits(frames[0]["center"][33 + n - 3, 1]) == 0                                       # -0 of the flipped view -> +0
    assert ref["status"][0, 33 + n - 4] == n - 4 and np.allclose(ref["angle"][0, n - 4], [0.6, 0.8], rtol=0, atol=1e-6)
    for k in (5, 6, 7, 8):
        assert m[0, n - k] == 1 and m[0, 33 + n - k] == 1                                       # invalid boxes: singletons
    assert m[0, n - 9] == 2 and m[0, n - 10] == 2
    assert (ref["status"][1] != N.NO_CANDIDATE).all()
    views3, _, _ = R.shape_case(3, 65, 3, 8, (False, True, False), "3d")
    ref3 = R.shape_reference(3, 65, 3, 8, (False, True, False), "3d", "max")
    assert (ref3["status"][2] == N.NO_CANDIDATE).all() and ref3["counts"][2] == 0
    _, frames3, _ = R.shape_case(3, 65, 3, 8, (False, True, False), "3d")
    st, cls = ref3["status"][1], frames3[1]["cls"]
    cand = sorted((m for m in range(len(st)) if st[m] >= -1), key=lambda m: (-float(cls[m].max()), m))
    pos = {m: i for i, m in enumerate(cand)}
    assert any(pos[m] // 64 != pos[int(st[m])] // 64 for m in cand if st[m] >= 0)               # a cluster straddles a block of 64
