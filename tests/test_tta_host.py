"""Host side of the test-time augmentation (dpft_amd/evaluation/tta.py): the config key, the evaluator's and the trainer's order of
calls with a stub model and stub launches, and the argument checks of the C-ABI entries (made before any launch).  No GPU."""
import ctypes as C

import pytest
import torch

from dpft_amd.evaluation.tta import TestTimeAugmentation as TTA

FOV = {"x": [0.0, 72.0], "y": [-6.4, 6.4], "z": [-2.0, 6.0], "azimuth": [-50, 50]}


def _cfg(spec, fov=FOV, resolution=None):
    cfg = {"evaluate": {"tta": spec}, "data": {"fov": fov}, "model": {"head": {"num_classes": 8}}}
    if resolution is not None:
        cfg["model"]["querent"] = {"resolution": resolution}
    return cfg


def test_from_config_absent_or_false_gives_none():
    assert TTA.from_config({}) is None and TTA.from_config({"evaluate": {}}) is None
    assert TTA.from_config(_cfg(None)) is None and TTA.from_config(_cfg(False)) is None


def test_from_config_true_gives_the_defaults():
    tta = TTA.from_config(_cfg(True))
    assert tta.view_specs == [(False, 1.0), (True, 1.0)] and tta.T == 2 and tta.flips == [False, True]
    assert (tta.iou, tta.kind, tta.score, tta.min_score) == (0.3, "bev", "mean", 0.0)
    assert TTA.from_config(_cfg({})).view_specs == tta.view_specs


def test_from_config_accepts_the_documented_dict():
    tta = TTA.from_config(_cfg({"views": [{"flip": True}, {"zoom": 1.1}, {"flip": True, "zoom": 0.9}], "iou": 0.5, "kind": "3d",
                                "score": "max", "min_score": 0.25}, resolution=[16, 16, 1]))
    assert tta.view_specs == [(False, 1.0), (True, 1.0), (False, 1.1), (True, 0.9)] and tta.T == 4
    assert (tta.iou, tta.kind, tta.score, tta.min_score) == (0.5, "3d", "max", 0.25)
    assert TTA.from_config(_cfg({"views": [{"zoom": 2}, {"zoom": 0.5}]})).view_specs[1:] == [(False, 2.0), (False, 0.5)]


@pytest.mark.parametrize("spec", [
    {"veiws": [{"flip": True}]}, {"iou": 0.3, "class_agnostic": False}, {"max_det": 5}, "flip", 1, [{"flip": True}],
    {"views": []}, {"views": {"flip": True}}, {"views": [{"flip": True}] * 4}, {"views": None},
    {"views": [{}]}, {"views": [{"flip": False}]}, {"views": [{"zoom": 1.0}]}, {"views": [{"flip": False, "zoom": 1}]},
    {"views": [{"flip": 1}]}, {"views": [{"flip": "yes"}]}, {"views": [{"zoom": 0.4}]}, {"views": [{"zoom": 2.5}]},
    {"views": [{"zoom": "1.1"}]}, {"views": [{"zoom": True}]}, {"views": [{"zoom": float("nan")}]}, {"views": [{"shift": 0.1}]},
    {"views": ["flip"]},
    {"score": "sum"}, {"score": None}, {"score": 0}, {"kind": "BEV"}, {"kind": "2d"}, {"kind": 0},
    {"iou": 0.0}, {"iou": 1.0}, {"iou": -0.1}, {"iou": "0.3"}, {"iou": True}, {"iou": None}, {"iou": float("nan")},
    {"min_score": -0.1}, {"min_score": None}, {"min_score": "0"}, {"min_score": True}, {"min_score": float("nan")},
    {"min_score": float("inf")},
])
def test_from_config_rejects_unknown_keys_and_bad_values(spec):
    with pytest.raises(ValueError, match="tta"):
        TTA.from_config(_cfg(spec))


def test_a_flipped_view_needs_a_symmetric_field_of_view():
    for fov in (dict(FOV, y=[-6.4, 8.0]), dict(FOV, azimuth=[-40, 50])):
        with pytest.raises(ValueError, match=r"evaluate\.tta.*symmetric"):
            TTA.from_config(_cfg(True, fov=fov))
        assert TTA.from_config(_cfg({"views": [{"zoom": 1.1}]}, fov=fov)).T == 2      # no flipped view: nothing to check
    assert TTA.from_config(_cfg(True, fov=None)).T == 2


def test_more_than_1024_candidates_are_refused_with_both_numbers():
    assert TTA.from_config(_cfg(True, resolution=[20, 20, 1])).T == 2
    with pytest.raises(ValueError, match=r"T = 3 .*N = 400"):
        TTA.from_config(_cfg({"views": [{"flip": True}, {"zoom": 1.1}]}, resolution=[20, 20, 1]))
    with pytest.raises(ValueError, match=r"T = 2 .*N = 513"):
        TTA().check_candidates(513)
    TTA().check_candidates(512)


def test_evaluator_and_trainer_build_no_tta_unless_the_key_is_set():
    import inspect
    from dpft_amd.evaluation import DataParallelEvaluator
    from dpft_amd.training.trainer import DataParallelTrainer
    assert DataParallelEvaluator(device="cpu").tta is None
    tta = TTA(iou=0.4)
    assert DataParallelEvaluator(device="cpu", tta=tta).tta is tta
    for cls in (DataParallelEvaluator.from_config, DataParallelTrainer.__init__):
        src = inspect.getsource(cls)
        assert 'get("tta")' in src and src.index('get("tta")') < src.index("import TestTimeAugmentation")      # imported under the key only


class _Stub(TTA):
    """Concatenates the views (the flipped ones negated in y and sin) without a device; counts its launches."""

    def views(self, data):
        self.log.append(("views", data))
        return [data] + [dict(data, view=t) for t in range(1, self.T)]

    def _launch(self, views):
        self.log.append(("fuse", len(views)))
        assert all(t.is_contiguous() and t.dtype == torch.float32 for v in views for t in v)
        B, N, _ = views[0][0].shape
        M = self.T * N
        cat = [torch.cat([v[i] for v in views], 1) for i in range(4)]
        z = torch.zeros((B, M), dtype=torch.int32)
        return (z - 1, z - 1, torch.full((B,), M, dtype=torch.int32), z + 1) + tuple(cat)


class _Model:
    def __init__(self, log):
        self.log = log

    def eval(self):
        pass

    def __call__(self, data):
        self.log.append(("model", data.get("view", 0), data.get("condition")))
        torch.manual_seed(data.get("view", 0))
        return {"center": torch.randn(2, 6, 3), "class": torch.randn(2, 6, 4), "size": torch.rand(2, 6, 3) + 0.5,
                "angle": torch.randn(2, 6, 2), "extra": data.get("view", 0)}


def test_fuse_returns_a_dict_of_the_type_and_key_order_of_view_0_with_t_n_rows():
    log = []
    tta = _Stub(views=[{"flip": True}, {"zoom": 1.5}])
    tta.log = log
    out = tta(_Model(log), {"x": 1})
    assert [e[0] for e in log] == ["views", "model", "model", "model", "fuse"] and [e[1] for e in log[1:4]] == [0, 1, 2]
    assert list(out) == ["center", "class", "size", "angle", "extra"] and out["extra"] == 0
    assert [tuple(out[k].shape) for k in ("class", "center", "size", "angle")] == [(2, 18, 4), (2, 18, 3), (2, 18, 3), (2, 18, 2)]
    status, order, counts, members = tta.clusters([_Model([])({"view": t}) for t in range(3)])
    assert status.shape == members.shape == (2, 18) and counts.tolist() == [18, 18]
    with pytest.raises(ValueError, match="3 views"):
        tta.fuse([_Model([])({})] * 2)
    with pytest.raises(ValueError, match="view 1"):
        tta.fuse([_Model([])({}), dict(_Model([])({}), angle=torch.randn(2, 6, 3)), _Model([])({})])


def test_cpu_tensors_are_refused_by_the_real_launcher():
    from dpft_amd.hip.lib import HipLibraryError
    out = _Model([])({})
    with pytest.raises(HipLibraryError, match="device tensors"):
        TTA().fuse([out, out])


def test_the_evaluator_fuses_before_the_nms_and_a_condition_takes_the_same_path():
    from dpft_amd.evaluation import DataParallelEvaluator
    log = []

    class Nms:
        def suppress(self, output):
            log.append(("nms", tuple(output["class"].shape)))
            return dict(output, suppressed=True)

    class Robustness:
        names = ["fog"]

        @staticmethod
        def scalar_key(key, name):
            return f"{key}/cond={name}"

        def apply(self, name, data, first_frame):
            log.append(("degrade", name))
            return dict(data, condition=name)

    def metric(output, labels):
        log.append(("metric", tuple(output["class"].shape), output.get("suppressed")))
        return {"m": torch.tensor(1.0)}

    def exporter(output, labels, step, dst):
        log.append(("export", tuple(output["class"].shape)))

    tta = _Stub()
    tta.log = log
    ev = DataParallelEvaluator(metric=metric, exporter=exporter, device="cpu", nms=Nms(), robustness=Robustness(), tta=tta)
    scalars = ev.evaluate_one_epoch(0, _Model(log), [({"x": torch.zeros(2, 1)}, [{}, {}])], dst="unused", shard_start=0)
    assert scalars == {"m": 1.0, "m/cond=fog": 1.0}
    kinds = [e[0] for e in log]
    assert kinds == ["views", "model", "model", "fuse", "nms", "metric", "export",
                     "degrade", "views", "model", "model", "fuse", "nms", "metric"]
    assert log[4] == ("nms", (2, 12, 4)) and log[5] == ("metric", (2, 12, 4), True) and log[6] == ("export", (2, 12, 4))
    assert log[8][1]["condition"] == "fog" and [e[2] for e in log[9:11]] == ["fog", "fog"]      # the views of the DEGRADED batch


def _validate_with(tta, nms=None):
    """``DataParallelTrainer._validate_one_epoch`` itself on a stand-in for the trainer (the pattern of tests/test_nms_host.py)."""
    import types
    from dpft_amd.training.trainer import DataParallelTrainer
    log, seen = [], {}
    if tta is not None:
        tta.log = log

    class Loss:
        def eval(self):
            pass

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

    me = types.SimpleNamespace(model=_Model(log), loss_fn=Loss(), eval_fn=metric, dataset_ap=AP(), nms=nms, tta=tta, logging=None,
                               rank=0, device=torch.device("cpu"), _dict_to=lambda d: d, _rank_mean=lambda d: d, _log=None)
    res = DataParallelTrainer._validate_one_epoch(me, 0, [({"x": torch.zeros(2, 1)}, [{}, {}])])
    assert res == {"loss": 1.0, "loss_center": 2.0, "mAP": 0.5, "mAP_bev@0.3": 0.25}
    return log, seen


def test_trainer_validation_feeds_the_loss_view_0_and_the_consumers_the_fused_dict():
    log, seen = _validate_with(_Stub())
    assert [e[0] for e in log] == ["views", "model", "model", "fuse"]
    assert tuple(seen["loss"]["class"].shape) == (2, 6, 4) and seen["loss"]["extra"] == 0
    assert seen["metric"] is seen["ap"] and tuple(seen["metric"]["class"].shape) == (2, 12, 4)
    assert torch.equal(seen["metric"]["class"][:, :6], seen["loss"]["class"])


def test_trainer_validation_without_tta_hands_the_raw_dict_on():
    log, seen = _validate_with(None)
    assert [e[0] for e in log] == ["model"] and seen["loss"] is seen["metric"] and seen["metric"] is seen["ap"]


def test_cabi_argument_checks_come_before_any_launch():
    from dpft_amd.hip.lib import TtaViews, lib
    assert lib.dpft_tta_scratch_bytes(1, 512, 2) > 0 and lib.dpft_tta_scratch_bytes(1, 512, 2) == lib.dpft_nms_scratch_bytes(1, 1024)
    assert lib.dpft_tta_scratch_bytes(4, 400, 2) == lib.dpft_nms_scratch_bytes(4, 800) and lib.dpft_tta_scratch_bytes(0, 400, 2) == 0
    assert lib.dpft_tta_scratch_bytes(1, 513, 2) == -1
    msg = lib.dpft_last_error()
    assert b"513" in msg and b"T 2" in msg and b"1024" in msg
    assert lib.dpft_tta_scratch_bytes(1, 8, 1) == -1 and b"T 1" in lib.dpft_last_error()
    assert lib.dpft_tta_scratch_bytes(1, 8, 5) == -1 and b"T 5" in lib.dpft_last_error()
    assert lib.dpft_tta_scratch_bytes(1, 256, 4) > 0 and lib.dpft_tta_scratch_bytes(1, 257, 4) == -1
    p = [C.c_void_p(256 * (i + 1)) for i in range(16)]      # never read: every call below is refused or has nothing to do

    def table(T=2, null=None):
        t = TtaViews()
        for i in range(T):
            t.cls[i], t.center[i], t.size[i], t.angle[i] = 4096 * (i + 1), 4096 * (i + 1) + 1024, 4096 * (i + 1) + 2048, 4096 * (i + 1) + 3072
        if null is not None:
            t.size[null] = None
        return t

    def gather(T=2, B=1, N=4, Cn=3, views=None, ptrs=p, tab=True):
        views = table(min(max(T, 0), 4)) if views is None else views
        return lib.dpft_tta_gather_f32(C.byref(views) if tab else None, T, ptrs[0], ptrs[1], ptrs[2], ptrs[3], B, N, Cn, None)

    assert gather(B=0) == 0 and gather(N=0) == 0
    assert gather(T=1) == -1 and gather(T=5) == -1 and b"T 5" in lib.dpft_last_error()
    assert gather(N=513) == -1 and b"513" in lib.dpft_last_error()
    assert gather(Cn=17) == -1 and b"C <= 16" in lib.dpft_last_error() and gather(Cn=1) == -1
    assert gather(tab=False) == -1 and b"null" in lib.dpft_last_error()
    assert gather(views=table(2, null=1)) == -1 and b"view 1" in lib.dpft_last_error()
    assert gather(ptrs=[None] + p[1:]) == -1 and b"null" in lib.dpft_last_error()
    assert gather(ptrs=[C.c_void_p(4096)] + p[1:]) == -1 and b"alias" in lib.dpft_last_error()

    def vote(T=2, B=1, N=4, Cn=3, score=0, ptrs=p):
        return lib.dpft_tta_vote_f32(ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], score, T, ptrs[5], ptrs[6], ptrs[7], ptrs[8],
                                     ptrs[9], B, N, Cn, None)

    assert vote(B=0) == 0 and vote(N=0) == 0
    assert vote(T=1) == -1 and vote(T=5) == -1 and vote(N=513) == -1 and b"513" in lib.dpft_last_error()
    assert vote(Cn=17) == -1 and b"C <= 16" in lib.dpft_last_error()
    assert vote(score=2) == -1 and b"score" in lib.dpft_last_error()
    for i in range(10):
        assert vote(ptrs=p[:i] + [None] + p[i + 1:]) == -1 and b"null" in lib.dpft_last_error(), i
    assert vote(ptrs=p[:6] + [p[0]] + p[7:]) == -1 and b"alias" in lib.dpft_last_error()
    assert vote(ptrs=p[:4] + [C.c_void_p(264)] + p[5:]) == -1 and b"alignment" in lib.dpft_last_error()
