"""LearnableQueries (src/dprt/models/queries/learnable.py) on the host: seeded initialisation, forward and backward against
what the REFERENCE's own module gives (tests/golden/learnable_queries.npz, written by tools/gen_learnable_queries_golden.py),
the model / state_dict plumbing, checkpoints, and the C-ABI argument checks of the kernels behind it."""
import copy
import ctypes as C

import pytest
import torch

from dpft_amd.models.queries import build_querent
from dpft_amd.models.queries.learnable import LearnableQueries
from oracle import dprt_oracle as O
from tests.test_oracle_golden import FUSER_CFG, T, _fuser_inputs, close

KRADAR_GRID = dict(resolution=[20, 20, 1], minimum=[4, -50, 0], maximum=[72, 50, 0], transformation="spher2cart")


def _seeded(q_init=None, seed=7):
    torch.manual_seed(seed)
    return build_querent("learnable_querent", dict(KRADAR_GRID, q_init=q_init))


def test_seeded_init_and_forward_equal_the_reference_bit_for_bit(golden):
    g = golden("learnable_queries.npz")
    q = _seeded()
    assert isinstance(q, LearnableQueries) and isinstance(q.queries, torch.nn.Parameter)
    assert tuple(q.queries.shape) == (400, 3) and q.q_init == "uniform_"
    assert torch.equal(q.queries.detach(), T(g["queries"]))
    out = q({"x": torch.zeros(2, 5), "y": torch.zeros(7, 1)})              # the batch size comes from the first entry
    assert list(out.keys()) == ["center"] and out["center"].requires_grad
    assert torch.equal(out["center"].detach(), T(g["center"]))
    assert torch.equal(q(torch.zeros(2, 1))["center"].detach(), T(g["center"]))
    assert torch.equal(q([torch.zeros(2, 1), torch.zeros(9)])["center"].detach(), T(g["center"]))
    # minimum == maximum == 0: uniform_(a=0, b=0) leaves the elevation at exactly 0, and with it z
    assert float(q.queries.detach()[:, 2].abs().max()) == 0.0 and float(out["center"].detach()[..., 2].abs().max()) == 0.0
    assert float(q.queries.detach()[:, 0].min()) >= 4 and float(q.queries.detach()[:, 0].max()) <= 72
    assert float(q.queries.detach()[:, 1].min()) >= -50 and float(q.queries.detach()[:, 1].max()) <= 50


def test_other_initialisers_go_through_torch_nn_init():
    q = _seeded("normal_", seed=3)
    torch.manual_seed(3)
    want = torch.nn.init.normal_(torch.empty(400, 3))
    assert torch.equal(q.queries.detach(), want)
    with pytest.raises(AttributeError):
        build_querent("learnable_querent", dict(KRADAR_GRID, q_init="no_such_init_"))
    plain = LearnableQueries([5, 2], [0.0, 1.0], [1.0, 2.0])                  # no transformation, two dimensions
    assert isinstance(plain.transformation, torch.nn.Identity)
    assert tuple(plain(torch.zeros(3, 1))["center"].shape) == (3, 10, 2) and plain.kernel_mode() is None


def test_no_grad_centres_follow_the_parameter():
    """Under no_grad the centres may be kept, but never past a change of the parameter: an in-place edit, load_state_dict,
    or a write through raw pointers that announces itself with note_weights_changed()."""
    from dpft_amd.hip.lib import note_weights_changed
    q = _seeded()
    x = torch.zeros(2, 1)
    with torch.no_grad():
        a = q(x)["center"]
        assert q(x)["center"] is a and not a.requires_grad
        assert tuple(q(torch.zeros(3, 1))["center"].shape) == (3, 400, 3)
        q.queries.mul_(0.5)
        b = q(x)["center"]
        assert torch.equal(b, q.transformation(q.queries.unsqueeze(0).repeat(2, 1, 1))) and not torch.equal(a, b)
        q.load_state_dict({"queries": q.queries.detach() * 3})
        c = q(x)["center"]
        assert torch.equal(c, q.transformation(q.queries.unsqueeze(0).repeat(2, 1, 1))) and not torch.equal(b, c)
        q.queries.data.mul_(2.0)                                             # (no version bump)
        note_weights_changed()
        d = q(x)["center"]
        assert torch.equal(d, q.transformation(q.queries.unsqueeze(0).repeat(2, 1, 1))) and not torch.equal(c, d)
    assert q(x)["center"].requires_grad                                     # grad mode never hands out the kept tensor
    assert "_centers" not in copy.deepcopy(q).__dict__


def test_static_querent_output_is_unchanged(golden):
    q = build_querent("data_agnostic_static_querent", dict(KRADAR_GRID))
    out = q({"x": torch.zeros(2, 3)})["center"]
    close(out, golden("querent.npz")["center"], rtol=1e-6, atol_scale=1e-7)
    assert not out.requires_grad and q({"x": torch.zeros(2, 3)})["center"] is out


def _kradar_cfg(learnable: bool):
    from dpft_amd.configs import load_config
    cfg = copy.deepcopy(load_config("kradar"))
    cfg["model"]["backbones"]["camera_mono"]["name"] = "ResNet50"            # keep the CPU test light
    if learnable:
        cfg["model"]["querent"] = dict(KRADAR_GRID, name="learnable_querent", q_init="uniform_")
    return cfg


def test_state_dict_names_are_the_static_models_plus_the_parameter():
    from dpft_amd.models import build
    static = build("dprt", _kradar_cfg(False))
    learned = build("dprt", _kradar_cfg(True))
    assert isinstance(learned.querent, LearnableQueries)
    ks, kl = list(static.state_dict().keys()), list(learned.state_dict().keys())
    assert [k for k in kl if k != "querent.queries"] == ks and kl.count("querent.queries") == 1
    assert dict(learned.named_parameters())["querent.queries"].requires_grad


@pytest.mark.parametrize("tag", ["A", "B"])
def test_cpu_backward_equals_the_reference(golden, tag):
    """queries.grad of the reference's own LearnableQueries -> IMPFusion (fixture) against the CPU torch-op path of this
    package's querent.  The product decoder has no CPU path, so the decoder between the centres and the loss is the oracle's
    eager IMPFusion on the weights and inputs of fuser_small.npz; the gate is the oracle's own (test_fuser_grads).
    Cotangents A: fuser_grads.npz; B: the same with cot/center = 0 -- the gradient then arrives through the reference points
    alone."""
    g, gg, gq = golden("fuser_small.npz"), golden("fuser_grads.npz"), golden("learnable_queries.npz")
    sd, views, proj, shp = _fuser_inputs(g)
    q = _seeded()
    out = O.impfusion(views, shp, proj, q(torch.zeros(2, 1))["center"], sd, "fuser", FUSER_CFG)
    cot = {k: T(gg[f"cot/{k}"]) for k in out}
    if tag == "B":
        cot["center"] = torch.zeros_like(cot["center"])
    loss = sum((out[k] * cot[k]).sum() for k in out)
    close(loss.detach(), gq[f"loss_{tag}"], rtol=1e-4)
    loss.backward()
    close(q.queries.grad, gq[f"grad_{tag}"], rtol=2e-3, atol_scale=2e-4)
    assert float(q.queries.grad.abs().max()) > 0


def test_checkpoints_round_trip_and_the_reference_pickle_maps_to_the_learnable_querent(tmp_path):
    """Whole-module checkpoints with a learned querent, after the model of
    test_host.test_load_reads_reference_whole_module_checkpoint: this package's own torch.save(model) file and its EMA twin,
    and a file whose classes are the reference's (dprt.models.queries.learnable.LearnableQueries)."""
    from collections import OrderedDict
    from dpft_amd.models import build, load
    from dpft_amd.models.checkpoint import infer_config, read_foreign
    from tests.test_host import _ForeignClasses, _as_reference_tree, _foreign_tree
    cfg = _kradar_cfg(True)
    m = cfg["model"]
    torch.manual_seed(5)
    ours = build("dprt", cfg)
    with torch.no_grad():
        ours.querent(torch.zeros(2, 1))                                       # a kept tensor must not reach the pickle
    sd = ours.state_dict()
    for name in ("20240101-130000_checkpoint_0003.pt", "20240101-130000_checkpoint_0003_ema.pt"):
        torch.save(ours, str(tmp_path / name))
        again, epoch, stamp = load(str(tmp_path / name))
        assert (epoch, stamp) == (3, "20240101-130000") and type(again.querent) is LearnableQueries
        assert "_centers" not in again.querent.__dict__
        assert torch.equal(again.querent.queries, ours.querent.queries) and again.querent.queries.requires_grad
        assert list(again.state_dict().keys()) == list(sd.keys())
    classes = _ForeignClasses()
    ref = _as_reference_tree(ours, classes, skip=("backbones", "necks")).eval()
    assert type(ref.querent).__module__ == "dprt.models.queries.learnable"
    for kind, path, cname in (("backbones", "torchvision.models.resnet", "ResNet"),
                              ("necks", "torchvision.ops.feature_pyramid_network", "FeaturePyramidNetwork")):
        holder = torch.nn.ModuleDict()
        for v in m["inputs"]:
            pre = f"{kind}.{v}."
            holder[v] = _foreign_tree(OrderedDict((k[len(pre):], t) for k, t in sd.items() if k.startswith(pre)),
                                      classes, path, cname)
        ref._modules[kind] = holder.eval()
    ckpt = tmp_path / "20240101-120000_checkpoint_0042.pt"
    with classes:
        torch.save(ref, str(ckpt))
    assert b"dprt.models.queries.learnable" in ckpt.read_bytes()
    inferred = infer_config(read_foreign(str(ckpt)))["model"]["querent"]
    assert inferred == dict(KRADAR_GRID, name="learnable_querent", q_init="uniform_")
    model, epoch, _ = load(str(ckpt))
    assert epoch == 42 and type(model.querent) is LearnableQueries and not model.training
    got = model.state_dict()
    assert list(got.keys()) == list(sd.keys())
    for k in sd:
        assert torch.equal(got[k], sd[k]), k
    # q_init is read, not assumed
    foreign = read_foreign(str(ckpt))
    foreign.querent.__dict__["q_init"] = "normal_"
    assert infer_config(foreign)["model"]["querent"]["q_init"] == "normal_"
    del foreign.querent.__dict__["q_init"]
    with pytest.raises(ValueError, match="q_init"):
        infer_config(foreign)


def test_cabi_null_and_shape_checks_of_the_query_kernels():
    """Argument validation happens before any launch, so it is testable without a GPU."""
    from dpft_amd.hip.lib import SIGNATURES, HeadTrain, lib
    for name in ("dpft_query_center_fwd_f32", "dpft_query_center_bwd_f32", "dpft_ref_points_bwd_f32"):
        assert name in SIGNATURES and hasattr(lib.load(), name)
    err = lambda: lib.dpft_last_error()      # noqa: E731
    p = [4096 * (i + 1) for i in range(4)]                                    # never dereferenced: every call is refused
    assert lib.dpft_query_center_fwd_f32(None, 0, p[1], 2, 4, None) == -1 and b"query_center_fwd: null" in err()
    assert lib.dpft_query_center_fwd_f32(p[0], 0, None, 2, 4, None) == -1
    assert lib.dpft_query_center_fwd_f32(p[0], 3, p[1], 2, 4, None) == -1 and b"mode 3" in err()
    assert lib.dpft_query_center_fwd_f32(p[0], 2, p[1], 0, 4, None) == -1 and b"bad shape" in err()
    assert lib.dpft_query_center_fwd_f32(p[0], 2, p[1], 1 << 20, 1 << 10, None) == -1 and b"bad shape" in err()
    assert lib.dpft_query_center_bwd_f32(None, p[1], 0, p[2], 2, 4, None) == -1 and b"query_center_bwd: null" in err()
    assert lib.dpft_query_center_bwd_f32(p[0], None, 0, p[2], 2, 4, None) == -1
    assert lib.dpft_query_center_bwd_f32(p[0], p[1], 0, None, 2, 4, None) == -1
    assert lib.dpft_query_center_bwd_f32(p[0], p[1], -1, p[2], 2, 4, None) == -1 and b"mode -1" in err()
    assert lib.dpft_query_center_bwd_f32(p[0], p[1], 1, p[2], 2, 0, None) == -1 and b"bad shape" in err()
    assert lib.dpft_ref_points_bwd_f32(None, 1, 1, 1, None) == -1
    h = HeadTrain()
    h.num_classes = 1
    assert lib.dpft_ref_points_bwd_f32(C.byref(h), 1, 1, 1, None) == -1 and b"prev_center is null" in err()
    h.prev_center = p[0]
    assert lib.dpft_ref_points_bwd_f32(C.byref(h), 1, 1, 5, None) == -1 and b"bad arguments" in err()
    assert lib.dpft_ref_points_bwd_f32(C.byref(h), 1, 1, 1, None) == -1 and b"drefs / dcenter_prev is null" in err()
    h.drefs, h.dcenter_prev = p[1], p[2]
    assert lib.dpft_ref_points_bwd_f32(C.byref(h), 1, 1, 1, None) == -1 and b"projection inputs of view 0" in err()
    h.P[0], h.shape[0], h.p_rows[0], h.has_t[0] = p[3], p[3], 3, 1             # has_t without T
    assert lib.dpft_ref_points_bwd_f32(C.byref(h), 1, 1, 1, None) == -1 and b"projection inputs of view 0" in err()
    h.y3 = p[3]
    assert lib.dpft_ref_points_bwd_f32(C.byref(h), 1, 1, 1, None) == -1 and b"y3 must be null" in err()
