"""Host side of the rotated NMS (dpft_amd/evaluation/nms.py): the config key, the argument checks of the C-ABI entry (made before any
launch), the suppress() dict contract against a stubbed launcher, and the trainer's validation loop with that stub.  No GPU."""
import collections
import ctypes as C

import pytest
import torch

from dpft_amd.evaluation.nms import RotatedNMS


def _cfg(spec):
    return {"evaluate": {"nms": spec}, "model": {"head": {"num_classes": 8}}}


def test_from_config_absent_or_false_gives_none():
    assert RotatedNMS.from_config({}) is None
    assert RotatedNMS.from_config({"evaluate": {}}) is None
    assert RotatedNMS.from_config(_cfg(None)) is None
    assert RotatedNMS.from_config(_cfg(False)) is None


def test_from_config_true_gives_the_defaults():
    nms = RotatedNMS.from_config(_cfg(True))
    assert (nms.iou, nms.kind, nms.class_agnostic, nms.min_score, nms.max_det) == (0.3, "bev", False, None, None)
    assert (RotatedNMS.from_config(_cfg({})).iou, RotatedNMS().kind) == (0.3, "bev")


def test_from_config_accepts_a_dict_of_exactly_the_five_keys():
    nms = RotatedNMS.from_config(_cfg({"iou": 0.5, "kind": "3d", "class_agnostic": True, "min_score": 0, "max_det": 50}))
    assert (nms.iou, nms.kind, nms.class_agnostic, nms.min_score, nms.max_det) == (0.5, "3d", True, 0.0, 50)
    assert isinstance(nms.min_score, float)
    nms = RotatedNMS.from_config(_cfg({"min_score": None, "max_det": None}))
    assert nms.min_score is None and nms.max_det is None


@pytest.mark.parametrize("spec", [
    {"iuo": 0.5}, {"iou": 0.3, "roi": None}, "bev", 1, [0.3],
    {"iou": 0.0}, {"iou": 1.0}, {"iou": -0.1}, {"iou": "0.3"}, {"iou": True}, {"iou": None}, {"iou": float("nan")},
    {"kind": "BEV"}, {"kind": "2d"}, {"kind": 0}, {"kind": ["bev"]},
    {"class_agnostic": 1}, {"class_agnostic": "yes"}, {"class_agnostic": None},
    {"min_score": "0.1"}, {"min_score": True}, {"min_score": float("nan")},
    {"max_det": 0}, {"max_det": -3}, {"max_det": 2.0}, {"max_det": True}, {"max_det": "5"}, {"max_det": 1 << 31},
])
def test_from_config_rejects_unknown_keys_and_bad_values(spec):
    with pytest.raises(ValueError, match="nms"):
        RotatedNMS.from_config(_cfg(spec))


def test_evaluator_builds_no_nms_unless_the_key_is_set():
    from dpft_amd.evaluation import DataParallelEvaluator, RotatedNMS as exported
    assert exported is RotatedNMS
    ev = DataParallelEvaluator(device="cpu")
    assert ev.nms is None
    ev = DataParallelEvaluator(device="cpu", nms=RotatedNMS(iou=0.4))
    assert ev.nms.iou == 0.4


class _Stub(RotatedNMS):
    """Marks every odd query of the batch as suppressed by its left neighbour, without a device."""

    def _launch(self, cls, center, size, angle):
        self.seen = (cls, center, size, angle)
        B, N, _ = cls.shape
        status = torch.full((B, N), -1, dtype=torch.int32)
        status[:, 1::2] = torch.arange(0, N - 1, 2, dtype=torch.int32)[: N // 2]
        order = torch.full((B, N), -1, dtype=torch.int32)
        kept = torch.arange(0, N, 2, dtype=torch.int32)
        order[:, :kept.numel()] = kept
        counts = torch.full((B,), kept.numel(), dtype=torch.int32)
        cls_out = cls.clone()
        cls_out[:, 1::2, 0] = 9.0
        return status, order, counts, cls_out


@pytest.mark.parametrize("kind", [dict, collections.OrderedDict])
def test_suppress_returns_a_new_dict_of_the_same_type_and_key_order(kind):
    torch.manual_seed(0)
    out = kind()
    out["center"], out["class"], out["extra"] = torch.randn(2, 6, 3), torch.randn(2, 6, 4), "kept as it is"
    out["size"], out["angle"] = torch.rand(2, 6, 3) + 0.5, torch.randn(2, 6, 2)
    before = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    nms = _Stub()
    res = nms.suppress(out)
    assert type(res) is kind and res is not out and list(res) == list(out)
    for k in out:
        if k != "class":
            assert res[k] is out[k]
        if isinstance(out[k], torch.Tensor):
            assert torch.equal(out[k], before[k])                       # the input is not written to
    assert res["class"] is not out["class"] and res["class"].dtype == torch.float32
    assert torch.equal(res["class"][:, 0::2], out["class"][:, 0::2]) and bool((res["class"][:, 1::2, 0] == 9.0).all())
    assert all(t.is_contiguous() and t.dtype == torch.float32 for t in nms.seen)
    status, order, counts, cls_out = nms(out)
    assert status.shape == order.shape == (2, 6) and counts.tolist() == [3, 3] and torch.equal(cls_out, res["class"])


def test_launcher_hands_fp32_contiguous_tensors_and_checks_the_shapes():
    nms = _Stub()
    out = {"class": torch.randn(1, 4, 3, dtype=torch.float64).transpose(1, 2).contiguous().transpose(1, 2),
           "center": torch.randn(1, 4, 3), "size": torch.rand(1, 4, 3), "angle": torch.randn(1, 4, 2)}
    assert not out["class"].is_contiguous()
    nms(out)
    assert nms.seen[0].is_contiguous() and nms.seen[0].dtype == torch.float32
    with pytest.raises(ValueError, match="RotatedNMS"):
        nms(dict(out, angle=torch.randn(1, 4, 3)))
    with pytest.raises(ValueError, match="RotatedNMS"):
        nms(dict(out, center=torch.randn(1, 5, 3)))


def test_cpu_tensors_are_refused_by_the_real_launcher():
    from dpft_amd.hip.lib import HipLibraryError
    out = {"class": torch.randn(1, 4, 3), "center": torch.randn(1, 4, 3), "size": torch.rand(1, 4, 3), "angle": torch.randn(1, 4, 2)}
    with pytest.raises(HipLibraryError, match="device tensors"):
        RotatedNMS()(out)
    with pytest.raises(HipLibraryError, match="device tensors"):
        RotatedNMS().suppress(out)


def test_cabi_argument_checks_come_before_any_launch():
    from dpft_amd.hip.lib import lib
    assert lib.dpft_nms_scratch_bytes(4, 400) > 0 and lib.dpft_nms_scratch_bytes(0, 400) == 0 and lib.dpft_nms_scratch_bytes(3, 0) == 0
    assert lib.dpft_nms_scratch_bytes(1, 1024) % 16 == 0
    assert lib.dpft_nms_scratch_bytes(1, 1025) == -1 and b"1024" in lib.dpft_last_error()
    assert lib.dpft_nms_scratch_bytes(-1, 4) == -1
    p = [C.c_void_p(256 * (i + 1)) for i in range(9)]       # never read: every call below is refused or has nothing to do
    inf, big = float("inf"), 0x7FFFFFFF

    def call(iou=0.3, kind=0, agn=0, ms=-inf, md=big, B=1, N=4, Cn=3, ptrs=p):
        thr = None if iou is None else (C.c_double * 1)(iou)      # (a host pointer, like dataset_ap's thresholds)
        return lib.dpft_nms_f32(ptrs[0], ptrs[1], ptrs[2], ptrs[3], thr, kind, agn, ms, md, ptrs[4], ptrs[5], ptrs[6], ptrs[7],
                                ptrs[8], B, N, Cn, None)

    assert call(B=0) == 0 and call(N=0) == 0 and call(B=0, ptrs=[None] * 9) == 0
    assert call(N=1025) == -1 and b"1024" in lib.dpft_last_error()
    assert call(Cn=17) == -1 and call(Cn=1) == -1 and call(B=-1) == -1
    assert call(iou=0.0) == -1 and call(iou=1.0) == -1 and call(iou=float("nan")) == -1 and b"(0, 1)" in lib.dpft_last_error()
    assert call(iou=None) == -1 and b"null" in lib.dpft_last_error()
    assert call(kind=2) == -1 and b"kind" in lib.dpft_last_error()
    assert call(ms=float("nan")) == -1 and b"min_score" in lib.dpft_last_error()
    assert call(md=0) == -1 and b"max_det" in lib.dpft_last_error()
    assert call(ptrs=[None] + p[1:]) == -1 and b"null" in lib.dpft_last_error()
    assert call(ptrs=p[:8] + [p[0]]) == -1 and b"alias" in lib.dpft_last_error()
    assert call(ptrs=p[:4] + [C.c_void_p(264)] + p[5:]) == -1 and b"alignment" in lib.dpft_last_error()


def _validate_with(nms):
    """``DataParallelTrainer._validate_one_epoch`` itself on a stand-in for the trainer (stub model, loss, metric, DatasetAP)."""
    import types
    from dpft_amd.training.trainer import DataParallelTrainer
    raw = {"class": torch.randn(2, 6, 4), "center": torch.randn(2, 6, 3), "size": torch.rand(2, 6, 3) + 0.5, "angle": torch.randn(2, 6, 2)}
    seen = {}

    class Model:
        def eval(self):
            pass

        def __call__(self, data):
            return raw

    class Loss(Model):
        def __call__(self, output, labels):
            seen["loss"] = output
            return torch.tensor(1.0), {"center": torch.tensor(2.0)}

    class AP:
        def reset(self):
            pass

        def update(self, output, labels, first_frame):
            seen["ap"] = output

        def all_gather(self):
            pass

        def scalars(self):
            return {"mAP_bev@0.3": 0.25}

    def metric(output, labels):
        seen["metric"] = output
        return {"mAP": torch.tensor(0.5)}

    me = types.SimpleNamespace(model=Model(), loss_fn=Loss(), eval_fn=metric, dataset_ap=AP(), nms=nms, logging=None, rank=0,
                               device=torch.device("cpu"), _dict_to=lambda d: d, _rank_mean=lambda d: d, _log=None)
    res = DataParallelTrainer._validate_one_epoch(me, 0, [({"x": torch.zeros(2, 1)}, [{}, {}])])
    assert res == {"loss": 1.0, "loss_center": 2.0, "mAP": 0.5, "mAP_bev@0.3": 0.25}
    return raw, seen


def test_trainer_validation_feeds_metric_and_dataset_ap_the_suppressed_dict_and_the_loss_the_raw_one():
    raw, seen = _validate_with(_Stub())
    assert seen["loss"] is raw
    assert seen["metric"] is seen["ap"] and seen["metric"] is not raw and list(seen["metric"]) == list(raw)
    assert all(seen["metric"][k] is raw[k] for k in raw if k != "class")
    assert bool((seen["metric"]["class"][:, 1::2, 0] == 9.0).all()) and not bool((raw["class"][:, 1::2, 0] == 9.0).any())


def test_trainer_validation_without_nms_hands_the_raw_dict_on():
    raw, seen = _validate_with(None)
    assert seen["loss"] is raw and seen["metric"] is raw and seen["ap"] is raw
