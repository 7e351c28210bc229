"""The fp64 restatement of the rotated NMS (tests/nms_ref.py) on hand-made cases whose answers are known without it, and its seeded
case builder: every case the GPU tests use terminates under the builder's two conditions."""
import numpy as np
import pytest

from tests import dataset_ap_ref as G
from tests import nms_ref as R


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_builder_terminates_on_every_seeded_case(name):
    frames, params, ref = R.shape_case(name)
    N, Ds, C, _layout, _ = R.SHAPES[name]
    assert len(frames) == len(Ds) and all(f["cls"].shape == (N, C) for f in frames)
    for f, D in zip(frames, Ds):
        assert R.candidates(f) == (0 if D == "nan" else D)
        assert float(np.nanmax(f["size"])) < 100 and float(np.min(f["size"])) >= 0.5 and float(np.max(np.abs(f["center"]))) < 100
    assert R.violations(frames, **params) == []
    assert ref["status"].shape == (len(Ds), N) and ref["cls_out"].shape == (len(Ds), N, C)


@pytest.mark.parametrize("name", sorted(R.directed_cases()))
def test_directed_cases_give_the_statuses_written_down_by_hand(name):
    frames, params, ties, expected = R.directed_cases()[name]
    if not name.startswith("half_"):      # (exactly on the threshold on purpose: dyadic numbers, every operation exact on both sides)
        assert R.violations(frames, ties_allowed=ties, **params) == []
    res = R.run(frames, **params)
    if expected is not None:
        assert res["status"].tolist() == expected
    _invariants(frames, params, res)


def _invariants(frames, params, res):
    """What holds for every result whatever the geometry: order lists exactly the kept queries by (score desc, query asc), counts
    counts them, cls_out differs from cls only at [n, 0] of the rows taken out, which then read as background."""
    for b, f in enumerate(frames):
        st, cls = res["status"][b], f["cls"]
        kept = [n for n in range(len(st)) if st[n] == R.KEPT]
        arg = np.argmax(cls, 1)
        kept.sort(key=lambda n: (-float(cls[n, arg[n]]), n))
        assert res["counts"][b] == len(kept) and res["order"][b, :len(kept)].tolist() == kept
        assert np.all(res["order"][b, len(kept):] == -1)
        if params.get("max_det") is not None:
            assert len(kept) <= params["max_det"]
        out = res["cls_out"][b]
        for n in range(len(st)):
            if st[n] in (R.KEPT, R.NO_CANDIDATE):
                assert out[n].tobytes() == cls[n].tobytes()
            else:
                assert out[n, 1:].tobytes() == cls[n, 1:].tobytes() and out[n, 0] == cls[n, arg[n]]
                assert int(np.argmax(out[n])) == 0 and np.all(np.isfinite(out[n]) | ~np.isfinite(cls[n]))
            if st[n] >= 0:
                assert st[st[n]] in (R.KEPT, R.BEYOND_MAX_DET)      # a suppressed candidate suppresses nothing


def test_chain_keeps_the_third_box():
    frames, params, _, _ = R.directed_cases()["chain"]
    f = frames[0]
    iou = lambda m, n: G.iou_pair(f["center"][m], f["size"][m], f["angle"][m], f["center"][n], f["size"][n], f["angle"][n])[0]
    assert iou(0, 1) > 0.3 and iou(1, 2) > 0.3 and iou(0, 2) < 0.3
    assert R.run(frames)["status"].tolist() == [[-1, 0, -1]]


def test_half_area_containment_is_exactly_one_half_in_both_kinds():
    o, i = np.array(R.HALF_OUTER, dtype=np.float32), np.array(R.HALF_INNER, dtype=np.float32)
    assert G.iou_pair(o[:3], o[3:6], o[6:], i[:3], i[3:6], i[6:]) == (0.5, 0.5)
    for kind in R.KINDS:
        frames = R.directed_cases()[f"half_{kind}_at_0.5"][0]
        assert R.run(frames, iou=0.5, kind=kind)["status"].tolist() == [[-1, -1]]           # strictly greater: kept
        assert R.run(frames, iou=0.4999, kind=kind)["status"].tolist() == [[-1, 0]]


def test_blocks_case_crosses_the_block_boundaries_as_described():
    frames = R.directed_cases()["blocks"][0]
    st = R.run(frames)["status"][0]
    assert (st[70], st[130]) == (0, 0)              # a keeper of block 0 takes out candidates of blocks 1 and 2
    assert st[1] == 0 and st[80] == -1              # the would-be victim of a suppressed candidate stays
    assert st[5] == -1 and st[140] == 5             # the first KEPT suppressor is named, not the suppressed query 70
    assert np.sum(st == -1) == 200 - 4


@pytest.mark.parametrize("name", ["dense_d65", "disjoint_d129", "b3_c8_3d_agnostic", "b5_c2_3d"])
def test_bounding_box_shortcut_equals_the_clip_on_every_pair(name):
    frames, params, _ = R.shape_case(name)
    notes = {}
    R.run(frames, notes=notes, **params)
    n_far = 0
    for fr, f in zip(notes["frames"], frames):
        q = [n for n, _, _ in fr["cands"]]
        for a, m in enumerate(q):
            for n in q[a + 1:]:
                full = G.iou_pair(f["center"][m], f["size"][m], f["angle"][m], f["center"][n], f["size"][n], f["angle"][n])
                n_far += fr["boxes"].apart(m, n)
                assert (fr["boxes"].pair_iou(m, n, 0), fr["boxes"].pair_iou(m, n, 1)) == full
    assert n_far > 0
