"""Rotated NMS on the device (csrc/nms.hip, dpft_amd/evaluation/nms.py) against the fp64 restatement of tests/nms_ref.py: status,
order and counts must equal the reference's integers, cls_out its bit patterns -- no tolerance anywhere (the case builder keeps every
IoU 1e-8 away from the threshold; the cases that sit exactly on it use dyadic numbers, exact on both sides)."""
import numpy as np
import pytest
import torch

from tests import nms_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _output(frames):
    return {k: torch.from_numpy(np.stack([f[src] for f in frames])).to(DEV)
            for k, src in (("class", "cls"), ("center", "center"), ("size", "size"), ("angle", "angle"))}


def _run(output, params):
    from dpft_amd.evaluation.nms import RotatedNMS
    status, order, counts, cls_out = RotatedNMS(**params)(output)
    assert (status.dtype, order.dtype, counts.dtype, cls_out.dtype) == (torch.int32, torch.int32, torch.int32, torch.float32)
    return {"status": status.cpu().numpy(), "order": order.cpu().numpy(), "counts": counts.cpu().numpy(),
            "cls_out": cls_out.cpu().numpy()}


def _same(got, ref):
    for k in ("status", "order", "counts"):
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        assert np.array_equal(got[k], ref[k]), (k, np.argwhere(got[k] != ref[k])[:5].tolist())
    a, b = got["cls_out"].view(np.uint32), np.ascontiguousarray(ref["cls_out"]).view(np.uint32)
    assert a.shape == b.shape and np.array_equal(a, b), np.argwhere(a != b)[:5].tolist()


def _check(frames, params, ref):
    got = _run(_output(frames), params)
    print("kept", got["counts"].tolist(), "reference", ref["counts"].tolist(),
          "suppressed", [int((s >= 0).sum()) for s in got["status"]])
    _same(got, ref)
    return got


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_equal_to_the_reference_over_the_shapes(name):
    frames, params, ref = R.shape_case(name)
    _check(frames, params, ref)


@pytest.mark.parametrize("name", sorted(R.directed_cases()))
def test_directed_cases(name):
    frames, params, _ties, expected = R.directed_cases()[name]
    got = _check(frames, params, R.run(frames, **params))
    if expected is not None:
        assert got["status"].tolist() == expected
    if name == "blocks":
        st = got["status"][0]
        assert (st[70], st[130], st[1], st[80], st[5], st[140]) == (0, 0, 0, -1, -1, 5)


def test_more_than_1024_queries_are_refused():
    from dpft_amd.evaluation.nms import RotatedNMS
    from dpft_amd.hip.lib import HipLibraryError
    out = {"class": torch.zeros(1, 1025, 3, device=DEV), "center": torch.zeros(1, 1025, 3, device=DEV),
           "size": torch.ones(1, 1025, 3, device=DEV), "angle": torch.ones(1, 1025, 2, device=DEV)}
    with pytest.raises(HipLibraryError, match="1024"):
        RotatedNMS()(out)
    with pytest.raises(HipLibraryError, match="C <= 16"):
        RotatedNMS()({k: (v[:, :8].repeat(1, 1, 6)[:, :, :17] if k == "class" else v[:, :8]) for k, v in out.items()})


@pytest.mark.parametrize("shape", [(0, 5, 3), (2, 0, 3)])
def test_empty_batches_and_frames_without_queries(shape):
    B, N, C = shape
    got = _run({"class": torch.zeros(B, N, C, device=DEV), "center": torch.zeros(B, N, 3, device=DEV),
                "size": torch.zeros(B, N, 3, device=DEV), "angle": torch.zeros(B, N, 2, device=DEV)}, {})
    assert got["status"].shape == (B, N) and got["order"].shape == (B, N) and got["cls_out"].shape == (B, N, C)
    assert got["counts"].tolist() == [0] * B


@pytest.mark.parametrize("name", ["dense_d1024", "b5_c16_bev_agnostic", "b3_c8_max_det"])
def test_running_twice_gives_identical_bits(name):
    frames, params, _ = R.shape_case(name)
    out = _output(frames)
    _same(_run(out, params), _run(out, params))


@pytest.mark.parametrize("name", ["dense_d129", "b3_c8_3d_agnostic", "b1_c8_min_score", "b3_c8_max_det"])
def test_suppress_applied_to_its_own_output_keeps_the_same_set(name):
    from dpft_amd.evaluation.nms import RotatedNMS
    frames, params, ref = R.shape_case(name)
    nms, out = RotatedNMS(**params), _output(frames)
    once = nms.suppress(out)
    assert np.array_equal(once["class"].cpu().numpy().view(np.uint32), ref["cls_out"].view(np.uint32))
    assert all(once[k] is out[k] for k in out if k != "class") and list(once) == list(out)
    status, order, counts, cls_out = nms(once)
    assert np.array_equal(order.cpu().numpy(), ref["order"]) and np.array_equal(counts.cpu().numpy(), ref["counts"])
    st = status.cpu().numpy()
    assert np.array_equal(st == R.KEPT, ref["status"] == R.KEPT) and np.all(st[ref["status"] != R.KEPT] == R.NO_CANDIDATE)
    assert torch.equal(cls_out, once["class"])


def test_strided_and_fp64_inputs_go_through_contiguous_fp32_copies():
    from dpft_amd.evaluation.nms import RotatedNMS
    frames, params, ref = R.shape_case("b3_c8_bev")
    out = _output(frames)
    wide = torch.zeros((3, 70, 16), device=DEV)
    wide[:, :, :8] = out["class"]
    got = RotatedNMS(**params)(dict(out, **{"class": wide[:, :, :8], "center": out["center"].double()}))
    assert np.array_equal(got[0].cpu().numpy(), ref["status"])
    assert np.array_equal(got[3].cpu().numpy().view(np.uint32), ref["cls_out"].view(np.uint32))
