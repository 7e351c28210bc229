"""The test-time-augmentation fusion on the device (csrc/tta.hip, dpft_amd/evaluation/tta.py) against the fp64 restatement of
tests/tta_ref.py.  Everything is compared bit for bit as integer views: geometry and class rows of heads, members, rows below the
threshold and rows that are no candidate, and status, order, counts and members.  The two fp64 operations whose rounding both sides
must share, / and sqrt, are IEEE on the device as in numpy (DESIGN.md section 3 "Test-time augmentation" records the measurement:
0 ulp over these cases), so the fused rows of multi-member heads are held to the same rule as all others."""
import numpy as np
import pytest
import torch

from tests import tta_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = (("class", "cls"), ("center", "center"), ("size", "size"), ("angle", "angle"))
CASES = [(shape, flips) for shape in R.SHAPES for flips in R.flip_patterns(shape[2])]


def _outputs(views):
    return [{k: torch.from_numpy(np.stack([f[src] for f in view])).to(DEV) for k, src in KEYS} for view in views]


def _tta(flips, **params):
    from dpft_amd.evaluation.tta import TestTimeAugmentation
    # a zoom tells an unflipped listed view from the identity; the fusion never looks at it
    return TestTimeAugmentation(views=[{"flip": True} if f else {"zoom": 1.25} for f in flips[1:]], **params)


def _run(tta, outputs):
    status, order, counts, members = tta.clusters(outputs)
    fused = tta.fuse(outputs)
    assert [t.dtype for t in (status, order, counts, members)] == [torch.int32] * 4
    got = {"status": status, "order": order, "counts": counts, "members": members}
    got.update({src: fused[k] for k, src in KEYS})
    return {k: v.cpu().numpy() for k, v in got.items()}


def _ulps(a, b):
    """Largest distance in fp32 ulps between two arrays of finite floats of equal sign (monotone integer keys)."""
    ka, kb = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ka, kb = np.where(ka < 0, -(ka & 0x7FFFFFFF), ka), np.where(kb < 0, -(kb & 0x7FFFFFFF), kb)
    return int(np.abs(ka - kb).max()) if ka.size else 0


def _same(got, ref):
    for k in ("status", "order", "counts", "members"):
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        assert np.array_equal(got[k], ref[k]), (k, np.argwhere(got[k] != ref[k])[:5].tolist())
    multi = ref["members"] >= 2
    for k in ("cls", "center", "size", "angle"):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert a.shape == b.shape, (k, a.shape, b.shape)
        finite = multi[..., None] & np.isfinite(a) & np.isfinite(b)
        print(k, "largest distance on the rows of multi-member heads:", _ulps(a[finite], b[finite]), "fp32 ulp")
        ua, ub = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(ua, ub), (k, np.argwhere(ua != ub)[:5].tolist())


@pytest.mark.parametrize("score", R.SCORES)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape,flips", CASES, ids=[f"{s}-{''.join('01'[f] for f in fl)}" for s, fl in CASES])
def test_equal_to_the_reference_bit_for_bit(shape, flips, kind, score):
    B, N, T, C = shape
    views, _frames, params = R.shape_case(B, N, T, C, flips, kind)
    ref = R.shape_reference(B, N, T, C, flips, kind, score)
    got = _run(_tta(flips, score=score, **params), _outputs(views))
    print("heads", got["counts"].tolist(), "largest cluster", int(got["members"].max()))
    _same(got, ref)


def test_fuse_keeps_the_dict_type_the_key_order_and_the_other_keys_of_view_0():
    import collections
    views, _, params = R.shape_case(2, 33, 2, 3, (False, True), "bev")
    outs = _outputs(views)
    first = collections.OrderedDict([("center", outs[0]["center"]), ("extra", "view 0"), ("class", outs[0]["class"]),
                                     ("size", outs[0]["size"]), ("angle", outs[0]["angle"])])
    before = {k: v.clone() for k, v in outs[0].items()}
    fused = _tta((False, True), **params).fuse([first, dict(outs[1], extra="view 1")])
    assert type(fused) is collections.OrderedDict and list(fused) == list(first) and fused["extra"] == "view 0"
    assert tuple(fused["class"].shape) == (2, 66, 3) and tuple(fused["angle"].shape) == (2, 66, 2)
    assert all(torch.equal(outs[0][k].view(torch.int32), before[k].view(torch.int32)) for k in before)      # the inputs are not written to


def test_running_twice_gives_identical_bits():
    views, _, params = R.shape_case(2, 130, 4, 16, (False, True, False, True), "3d")
    tta, outs = _tta((False, True, False, True), **params), _outputs(views)
    a, b = _run(tta, outs), _run(tta, outs)
    for k in a:
        assert np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k],
                              b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k]), k


def test_strided_and_fp64_outputs_go_through_contiguous_fp32_copies():
    views, _, params = R.shape_case(2, 33, 2, 3, (False, True), "bev")
    ref = R.shape_reference(2, 33, 2, 3, (False, True), "bev", "mean")
    outs = _outputs(views)
    wide = torch.zeros((2, 33, 8), device=DEV)
    wide[:, :, :3] = outs[1]["class"]
    outs[1] = dict(outs[1], **{"class": wide[:, :, :3], "center": outs[1]["center"].double()})
    got = _run(_tta((False, True), **params), outs)
    _same(got, ref)


def test_more_than_1024_candidates_more_than_16_classes_and_a_wrong_number_of_views_are_refused():
    z = lambda n, c: {"class": torch.zeros(1, n, c, device=DEV), "center": torch.zeros(1, n, 3, device=DEV),
                      "size": torch.ones(1, n, 3, device=DEV), "angle": torch.ones(1, n, 2, device=DEV)}
    tta = _tta((False, True))
    with pytest.raises(ValueError, match=r"T = 2 .* N = 513"):
        tta.fuse([z(513, 3), z(513, 3)])
    with pytest.raises(ValueError, match="C <= 16"):
        tta.fuse([z(8, 17), z(8, 17)])
    with pytest.raises(ValueError, match="2 views"):
        tta.fuse([z(8, 3)])
    with pytest.raises(ValueError, match="view 1"):
        tta.fuse([z(8, 3), z(9, 3)])
    got = tta.fuse([z(0, 3), z(0, 3)])
    assert tuple(got["class"].shape) == (1, 0, 3)
