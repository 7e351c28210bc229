"""CPU-only checks: C-ABI surface, host-side mirror of the reference interface, configs."""
import copy
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden_digests():
    """Digests of what the reference's own code and files give (oracle/gen_golden.py reference_digests)."""
    with open(os.path.join(ROOT, "tests", "golden", "reference_digests.json")) as f:
        return json.load(f)


def test_cabi_exports_every_declared_symbol():
    from dpft_amd.hip.lib import LIB_PATH, SIGNATURES, lib
    header = open(os.path.join(ROOT, "include", "dpft_hip.h")).read()
    declared = set(re.findall(r"\b(dpft_[a-z0-9_]+)\s*\(", header))
    declared -= {"dpft_stream_t"}
    assert declared, "no declarations parsed"
    assert os.path.exists(LIB_PATH), "libdpft_hip.so not built (run __graft_entry__.build())"
    dll = lib.load()
    for name in sorted(declared):
        assert hasattr(dll, name), f"{name} declared in include/dpft_hip.h but not exported"
        assert name in SIGNATURES, f"{name} has no ctypes signature"
    assert set(SIGNATURES) == declared
    assert dll.dpft_version() >= 100


def test_cabi_argument_errors_are_reported():
    """Argument validation happens before any launch, so it is testable without a GPU."""
    import ctypes as C
    from dpft_amd.hip.lib import ConvDesc, lib
    bad = ConvDesc(1, 8, 8, 64, 64, 3, 3, 1, 1, 5, 5)       # OH/OW inconsistent
    assert lib.dpft_conv2d_workspace_bytes(C.byref(bad)) == -1
    assert b"inconsistent" in lib.dpft_last_error()
    rc = lib.dpft_xattn_fwd_f32(None, None, None, None, None, None, None, None, None, 1, 1, 4, 4, 4, None)
    assert rc != 0 and b"M=8" in lib.dpft_last_error()
    # compute-mode switch: 0 fp32 (default) | 1 bf16 operands | 2 three-term bf16 split; anything else is rejected
    assert lib.dpft_conv_get_compute() == 0
    assert lib.dpft_conv_set_compute(3) == -1 and b"conv_set_compute" in lib.dpft_last_error()
    assert lib.dpft_conv_set_compute(1) == 0 and lib.dpft_conv_get_compute() == 1
    assert lib.dpft_conv_set_compute(0) == 0 and lib.dpft_conv_get_compute() == 0
    # forward conv: combinations no kernel serves are refused before anything is launched (the pointers are never read)
    from dpft_amd.hip.lib import make_desc
    x, w, y, stats, bias, bnp, ws = (C.c_void_p(256 * (i + 1)) for i in range(7))
    d = make_desc(8, 56, 56, 64, 256, 1, 1, 1, 0)           # a streaming 1x1 problem: its statistics come in that kernel's tiling
    tr = C.c_int32(0)
    assert lib.dpft_conv2d_stats_tiles(C.byref(d), C.byref(tr)) == -(-8 * 56 * 56 // tr.value)
    rc = lib.dpft_conv2d_nhwc_fwd_f32(C.byref(d), x, w, bias, None, 0, y, stats, ws, None)
    assert rc == -1 and b"streaming 1x1" in lib.dpft_last_error()
    rc = lib.dpft_conv2d_nhwc_fwd_f32(C.byref(d), x, w, None, bnp, 0, y, stats, ws, None)
    assert rc == -1 and b"streaming 1x1" in lib.dpft_last_error()
    d16 = make_desc(2, 16, 16, 64, 128, 3, 3, 1, 1)
    d16.act16 = 2                                             # bf16 weights: no operand prologue
    rc = lib.dpft_conv2d_nhwc_fwd_f32(C.byref(d16), x, w, None, bnp, 1, y, None, ws, None)
    assert rc == -1 and b"act16 = 2" in lib.dpft_last_error()
    # inference epilogue: the output channels come four at a time (found by the geometry lattice, tests/conv_lattice.py)
    d66 = make_desc(2, 8, 8, 64, 66, 3, 3, 1, 1)
    rc = lib.dpft_conv2d_nhwc_fwd_bnact_f32(C.byref(d66), x, w, bnp, 1, None, y, ws, None)
    assert rc == -1 and b"conv fwd_bnact: K % 4 == 0 needed (K=66)" in lib.dpft_last_error()
    # weight gradient: the operand prologue exists in the vector kernels only
    rc = lib.dpft_conv2d_nhwc_wgrad_f32(C.byref(d66), x, y, bnp, 1, w, ws, None)
    assert rc == -1 and b"conv wgrad: fused prologue needs C % 32 == 0 and K % 4 == 0 (C=64, K=66)" in lib.dpft_last_error()


def test_bn_pass_entries_refuse_what_their_workers_refuse():
    """The storage-typed BatchNorm pass entries (dpft_*_any_f32, dpft_bn_act_sums_f32, dpft_cvt_f32_bf16): DPFT_ERR_ARG before
    anything is launched, so testable without a GPU (the pointers are never read)."""
    import ctypes as C
    from dpft_amd.hip.lib import lib
    p = [C.c_void_p(4096 * (i + 1)) for i in range(12)]
    err = lambda: lib.dpft_last_error()
    assert lib.dpft_bn_act_any_f32(p[0], p[1], None, None, 1, p[2], None, None, 8, 6, 0, None) == -1 and b"bn_act: bad arguments (K=6)" in err()
    assert lib.dpft_bn_act_any_f32(p[0], p[1], None, p[3], 1, p[2], None, None, 8, 8, 1, None) == -1 and b"res_bnp without res" in err()
    assert lib.dpft_bn_act_any_f32(p[0], p[1], None, None, 1, p[2], None, None, 8, 8, 2, None) == -1 and b"storage" in err()
    assert lib.dpft_bn_act_any_f32(None, p[1], None, None, 1, p[2], None, None, 8, 8, 0, None) == -1
    assert lib.dpft_bn_act_any_f32(C.c_void_p(4100), p[1], None, None, 1, p[2], None, None, 8, 8, 1, None) == -1 and b"aligned" in err()
    used = C.c_int32(7)
    a = (p[0], p[1], p[2], p[3], p[4], None, p[5])
    assert lib.dpft_bn_act_sums_f32(*a, None, None, None, 0.0, 1, p[6], None, 8, 8, C.byref(used), None) == -1 and used.value == 0
    assert b"without a residual" in err()
    assert lib.dpft_bn_act_sums_f32(p[0], None, p[2], None, p[4], None, None, None, None, None, 0.0, 1, p[6], None, 8, 8,
                                    C.byref(used), None) == -1 and b"without gamma" in err()
    assert lib.dpft_bn_act_sums_f32(p[0], None, None, None, None, None, None, None, None, None, 0.0, 1, p[6], None, 8, 8,
                                    C.byref(used), None) == -1
    assert lib.dpft_bn_act_sums_f32(*a[:5], None, None, None, None, None, 0.0, 1, p[6], None, 8, 10, C.byref(used), None) == -1
    assert lib.dpft_bn_bwd_reduce_any_f32(p[0], p[1], None, None, None, p[2], p[3], 8, 6, 0, None) == -1 and b"bn_bwd_reduce" in err()
    assert lib.dpft_bn_bwd_reduce_any_f32(p[0], None, None, None, None, p[2], p[3], 8, 8, 1, None) == -1
    ap = lambda **kw: lib.dpft_bn_bwd_apply_any_f32(p[0], p[1], None, None, None, p[2], p[3], p[4], p[5], None, None, kw.get("zb"),
                                                    kw.get("zn", 0), 8, kw.get("K", 8), kw.get("st", 0), 0, None)
    assert ap(K=6) == -1 and b"bn_bwd_apply" in err()
    assert ap(zn=4) == -1 and b"zero_buf" in err()
    assert ap(zb=p[4], zn=4) == -1 and b"must not be the sums" in err()
    assert ap(st=3) == -1
    assert lib.dpft_bn_relu_maxpool_any_f32(p[0], p[1], p[2], 1, 4, 4, 6, 2, 2, 0, None) == -1
    assert lib.dpft_bn_relu_maxpool_any_f32(p[0], p[1], p[2], 1, 4, 4, 8, 3, 2, 1, None) == -1 and b"PH/PW inconsistent" in err()
    assert lib.dpft_bn_relu_maxpool_bwd_any_f32(p[0], p[1], p[2], p[3], 1, 4, 4, 4, 3, 2, 0, None) == -1 and b"PH/PW inconsistent" in err()
    assert lib.dpft_bn_relu_maxpool_bwd_any_f32(p[0], p[1], p[2], p[3], 1, 4, 4, 6, 2, 2, 0, None) == -1
    assert lib.dpft_add_inplace_any_f32(p[0], p[1], 6, 1, None) == -1 and b"add_inplace" in err()
    assert lib.dpft_cvt_f32_bf16(p[0], p[1], 6, None) == -1 and lib.dpft_cvt_f32_bf16(None, p[1], 8, None) == -1
    assert lib.dpft_bn_last_form(None) == -1
    form = C.c_int32(-1)
    assert lib.dpft_bn_last_form(C.byref(form)) == 0 and form.value == 0          # nothing launched in this process


def test_head_train_entries_refuse_what_hd_fill_and_hd_check_proj_refuse():
    """dpft_head_train_fwd_f32 / _bwd_f32 / dpft_ref_points_bwd_f32 (decoder_train_h.hip): every refusal of hd_fill and
    hd_check_proj comes back as DPFT_ERR_ARG with a message before anything is launched (the pointers are never read)."""
    import ctypes as C
    from dpft_amd.hip.lib import HeadTrain, lib
    p = [4096 * (i + 1) for i in range(8)]
    err = lambda: lib.dpft_last_error()
    entries = (lib.dpft_head_train_fwd_f32, lib.dpft_head_train_bwd_f32, lib.dpft_ref_points_bwd_f32)

    def base():
        h = HeadTrain()
        h.prev_center, h.num_classes = p[0], 2
        return h
    for fn in entries:
        assert fn(None, 1, 1, 1, None) == -1 and err()
        for V in (0, 5):
            assert fn(C.byref(base()), 1, 1, V, None) == -1 and b"head_train: bad arguments" in err(), (fn, V)
        for ncls in (0, 17):
            h = base()
            h.num_classes = ncls
            assert fn(C.byref(h), 1, 1, 1, None) == -1 and b"num_classes must be in [1,16]" in err(), (fn, ncls)
        h = base()
        h.prev_center = None
        assert fn(C.byref(h), 1, 1, 1, None) == -1 and b"prev_center is null" in err(), fn

    # reference points wanted (forward: refs; backward: drefs; ref_points_bwd: always) with the projection inputs incomplete
    def wanting(which):
        h = base()
        if which == 0:
            h.refs = p[1]
        elif which == 1:
            h.y3, h.packed, h.red_w, h.drefs = p[1], p[2], p[3], p[1]
            for g in range(4):
                for k in range(3):
                    h.head_w[g][k] = p[4]
            h.dy3, h.dcenter_prev, h.rows = p[5], p[6], p[7]
        else:
            h.drefs, h.dcenter_prev = p[1], p[6]
        for v in range(2):
            h.P[v], h.shape[v], h.T[v], h.p_rows[v], h.has_t[v] = p[2], p[3], p[4], 3, 1
        return h
    for which, fn in enumerate(entries):
        for view in (0, 1):
            msg = b"projection inputs of view %d missing" % view
            for field, value in (("P", None), ("shape", None), ("p_rows", 2), ("T", None)):
                h = wanting(which)
                getattr(h, field)[view] = value
                assert fn(C.byref(h), 1, 1, 2, None) == -1 and msg in err(), (fn, view, field)
    h = wanting(2)
    h.y3 = p[1]
    assert lib.dpft_ref_points_bwd_f32(C.byref(h), 1, 1, 2, None) == -1 and b"y3 must be null" in err()
    # the backward without its outputs, the forward with y3 but without its outputs or weights
    h = wanting(1)
    h.rows = None
    assert lib.dpft_head_train_bwd_f32(C.byref(h), 1, 1, 2, None) == -1 and b"head_train_bwd: null output" in err()
    h = wanting(1)
    assert lib.dpft_head_train_fwd_f32(C.byref(h), 1, 1, 2, None) == -1 and b"head_train_fwd: null output" in err()
    h.head_w[3][2] = None
    assert lib.dpft_head_train_fwd_f32(C.byref(h), 1, 1, 2, None) == -1 and b"head weight 3.2 is null" in err()


def test_every_compute_entry_rejects_null_arguments():
    """Error behaviour of the boundary: every compute entry validates its arguments before touching the device and
    reports DPFT_ERR_ARG + a message through dpft_last_error() (no GPU needed; run in a child process because a missing
    check would be a crash)."""
    import subprocess
    import sys
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cabi_null_probe.py")], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])
    assert len(got) >= 44, sorted(got)
    for name, (rc, err) in got.items():
        assert rc == -1, (name, rc, err)                       # DPFT_ERR_ARG
        assert err and ":" in err, (name, err)                 # "<entry>: what was wrong"


def test_state_dict_layout_matches_reference_naming():
    from dpft_amd.configs import load_config
    from dpft_amd.models import build
    model = build("dprt", load_config("kradar"))
    sd = model.state_dict()
    n_params = sum(p.numel() for p in model.parameters())
    assert n_params == 89_892_084 + 2_208                       # SURVEY App. A (+ the un-cloned template head)
    assert sd["backbones.radar_bev.adjustment_layer.weight"].shape == (3, 6, 1, 1)
    assert "backbones.camera_mono.adjustment_layer.weight" not in sd
    assert sd["backbones.camera_mono.body.conv1.weight"].shape == (64, 3, 7, 7)
    assert sd["backbones.camera_mono.body.layer3.22.conv3.weight"].shape == (1024, 256, 1, 1)
    assert sd["backbones.camera_mono.body.layer2.0.downsample.0.weight"].shape == (512, 256, 1, 1)
    assert sd["backbones.camera_mono.body.layer2.0.downsample.1.running_var"].shape == (512,)
    assert sd["backbones.radar_front.body.layer3.5.bn2.num_batches_tracked"].dtype == torch.int64
    assert "backbones.radar_front.body.layer3.6.conv1.weight" not in sd          # ResNet-50 depth
    assert sd["necks.camera_mono.fpn.inner_blocks.0.0.weight"].shape == (16, 3, 1, 1)
    assert sd["necks.radar_bev.fpn.inner_blocks.4.0.bias"].shape == (16,)
    assert sd["necks.radar_bev.fpn.layer_blocks.2.0.weight"].shape == (16, 16, 3, 3)
    assert sd["fuser.mpfusion.fusion3.ml_fusion_layers.ms_deform_attn2.ms_deform_attn.sampling_offsets.weight"].shape == (320, 16)
    assert sd["fuser.mpfusion.fusion0.reduction_layer.weight"].shape == (16, 48)
    assert sd["fuser.heads.3.layers.class_head.6.weight"].shape == (2, 16)
    assert sd["head.layers.center_head.0.weight"].shape == (16, 16)
    bn = sum(1 for k in sd if k.endswith("running_mean"))
    assert bn == 104 + 53 + 53
    # conv weights live in the [Cout][kh][kw][Cin] physical layout the HIP kernels read
    w = model.backbones["camera_mono"].body.layer1[0].conv2.weight
    assert w.permute(0, 2, 3, 1).is_contiguous()


def test_fuser_state_dict_identical_to_reference(golden_digests):
    """Same state-dict layout (names, order, shapes) as the reference's IMPFusion, and the same deterministic
    initialisation (ring-pattern sampling offsets) -- against digests of the reference's own module
    (tests/golden/reference_digests.json, oracle/gen_golden.py reference_digests)."""
    from oracle import digests as D
    from dpft_amd.configs import load_config
    from dpft_amd.models.fusers import build_fuser
    from dpft_amd.models.heads import build_head
    cfg = load_config("kradar")
    comp, m = cfg["computing"], cfg["model"]
    ours = build_fuser(m["fuser"]["name"], dict(comp | m["fuser"]), head=build_head(m["head"]["name"], dict(comp | m["head"])))
    a, ref = ours.state_dict(), golden_digests["fuser"]
    # equal layouts: our checkpoint loads into the reference module unchanged (strict load_state_dict)
    assert D.state_layout_digest(a) == ref["state_layout"]
    k = "mpfusion.fusion0.ml_fusion_layers.ms_deform_attn0.ms_deform_attn.sampling_offsets.bias"
    assert D.tensor_digest(a[k]) == ref["sampling_offsets_bias"]


@pytest.mark.parametrize("name", ["kradar", "kradar_camera_mono", "kradar_radar_bev", "kradar_radar_front", "kradar_radar"])
def test_builtin_configs_equal_reference_jsons(name, tmp_path, golden_digests):
    """The built-in configs are the reference's config/<name>.json files with the backbone weights names blanked: ours with
    the weights name put back has the digest of the reference file's compared sections (tests/golden/reference_digests.json),
    and that file form loads as the reference's file does."""
    from oracle import digests as D
    from dpft_amd.configs import load_config
    ours = load_config(name)
    ref = json.loads(json.dumps(ours))
    for bb in ref["model"]["backbones"].values():
        assert bb["weights"] == ""
        bb["weights"] = "IMAGENET1K_V2"
    assert D.config_digest(ref) == golden_digests["configs"][name]
    path = str(tmp_path / (name + ".json"))
    with open(path, "w") as f:
        json.dump(ref, f)
    with pytest.warns(UserWarning, match="RANDOM initialisation"):            # explicit opt-in, never silent
        loaded = load_config(path, offline=True)
    assert loaded["model"] == ours["model"]
    assert load_config(path)["model"] == json.load(open(path))["model"]      # default: the JSON unchanged
    mapped = load_config(path, weight_files={"IMAGENET1K_V2": "/w/imagenet.pt"})
    assert all(bb["weights"] == "/w/imagenet.pt" for bb in mapped["model"]["backbones"].values())


def test_no_cpu_fallback():
    """The product path must fail loudly without a GPU / HIP library (no oracle, no eager fallback)."""
    from dpft_amd.configs import load_config
    from dpft_amd.models import build
    from dpft_amd.synthetic import make_batch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    cfg = load_config("kradar_radar_front")
    model = build("dprt", cfg)
    batch = make_batch(cfg["model"]["inputs"], 1)
    with pytest.raises(RuntimeError, match="no CPU path|CUDA"):
        model(batch)
    import dpft_amd.models.dprt as d
    src = open(d.__file__).read() + open(os.path.join(ROOT, "dpft_amd", "hip", "ops.py")).read()
    assert "oracle" not in src


def test_oracle_camera_mono_cpu_plumbing():
    """BASELINE config[0]: kradar_camera_mono, batch 1, CPU forward of the restatement (reduced frame)."""
    from dpft_amd.configs import load_config
    from dpft_amd.models import build
    from dpft_amd.synthetic import make_batch
    from oracle import dprt_oracle as O
    cfg = load_config("kradar_camera_mono")
    cfg["model"]["backbones"]["camera_mono"]["name"] = "ResNet50"
    torch.manual_seed(0)
    model = build("dprt", cfg)
    batch = make_batch(["camera_mono"], 1, shapes={"camera_mono": (72, 128, 3)})
    out = O.dprt_forward(model.state_dict(), cfg, batch, train=False)
    assert list(out) == ["center", "size", "angle", "class"]
    assert out["center"].shape == (1, 400, 3) and out["class"].shape == (1, 400, 2)
    assert all(torch.isfinite(v).all() for v in out.values())


def test_synthetic_batch_contract():
    from dpft_amd.synthetic import make_batch, make_labels
    b = make_batch(["camera_mono", "radar_bev", "radar_front"], 4)
    assert list(b)[0] == "camera_mono" and b["camera_mono"].shape == (4, 512, 910, 3)
    assert b["radar_bev"].shape == (4, 256, 107, 6) and b["radar_front"].shape == (4, 37, 107, 6)
    assert b["camera_mono_shape"].tolist()[0] == [720, 1280, 3] and b["camera_mono_shape"].dtype == torch.int64
    assert not b["label_to_camera_mono_t"].any() and b["label_to_radar_bev_p"].shape == (4, 3, 4)
    b2 = make_batch(["camera_mono"], 4)
    assert torch.equal(b["camera_mono"], b2["camera_mono"])
    lab = make_labels(4)
    assert len(lab) == 4 and all(1 <= l["gt_center"].shape[0] <= 8 for l in lab)


class _ForeignClasses:
    """Classes that pickle under class paths which are NOT importable when the file is read (the reference's ``dprt.*``,
    torchvision's): inside the ``with`` block every module of their dotted paths is a stand-in in ``sys.modules`` (what the
    pickler looks the class up in), removed again on exit."""

    def __init__(self):
        self.made, self.saved = {}, {}

    def cls(self, module_path, name):
        if (module_path, name) not in self.made:
            self.made[(module_path, name)] = type(name, (torch.nn.Module,), {"__module__": module_path})
        return self.made[(module_path, name)]

    def __enter__(self):
        import sys
        import types
        for (path, name), cls in self.made.items():
            parts = path.split(".")
            for i in range(1, len(parts) + 1):
                p = ".".join(parts[:i])
                if p not in self.saved:
                    self.saved[p] = sys.modules.get(p)
                    sys.modules[p] = types.ModuleType(p)
            setattr(sys.modules[path], name, cls)
        return self

    def __exit__(self, *exc):
        import sys
        for p, old in self.saved.items():
            if old is None:
                sys.modules.pop(p, None)
            else:
                sys.modules[p] = old
        return False


def _foreign_tree(state_dict, classes, module_path, cls_name):
    """A module tree whose classes pickle as ``<module_path>.<cls_name>`` holding exactly ``state_dict`` -- the shape of what
    torch.save(model) writes for the third-party parts (torchvision ResNet / FPN) of a reference checkpoint."""
    cls = classes.cls(module_path, cls_name)
    root = cls()
    for key, t in state_dict.items():
        node, parts = root, key.split(".")
        for part in parts[:-1]:
            if part not in node._modules:
                node.add_module(part, cls())
            node = node._modules[part]
        if parts[-1] in ("running_mean", "running_var", "num_batches_tracked"):
            node.register_buffer(parts[-1], t.clone())
        else:
            node.register_parameter(parts[-1], torch.nn.Parameter(t.clone()))
    return root


def _as_reference_tree(mod, classes, skip=()):
    """What the reference's own module tree pickles as, made from this package's, which mirrors it class for class and
    attribute for attribute: every ``dpft_amd.models.X.Y`` becomes ``dprt.models.X.Y``, each module keeps its pickled state
    minus this package's own caches (``_tables`` / ``_cache``: the reference has none).  The top-level children in ``skip``
    are left empty.  The test pins the result to the reference's tree by digest."""
    from collections import OrderedDict
    cls = type(mod)
    if cls.__module__.startswith("dpft_amd."):
        cls = classes.cls("dprt." + cls.__module__[len("dpft_amd."):], cls.__qualname__)
    st = dict(mod.__getstate__())
    st.pop("_tables", None)
    st.pop("_cache", None)
    obj = cls.__new__(cls)
    obj.__dict__.update(st)
    obj.__dict__["_parameters"] = dict(mod._parameters)
    obj.__dict__["_buffers"] = dict(mod._buffers)
    obj.__dict__["_modules"] = OrderedDict((k, torch.nn.ModuleDict() if k in skip else _as_reference_tree(c, classes))
                                           for k, c in mod._modules.items())
    return obj


def test_load_reads_reference_whole_module_checkpoint(tmp_path, golden_digests):
    """f-3 remainder (VERDICT r1 missing #1): ``dpft_amd.models.load`` on a ``torch.save(model)`` file whose classes are
    the REFERENCE's (dprt.models.dprt.DPRT, IMPFusion, MLFusion, MSDeformAttn, LinearDetectionHead, the querent, the
    embeddings -- the reference's module tree, equal by digest to what the reference itself builds) and torchvision's
    (class paths that are not importable when the file is read): the rebuilt dpft_amd model has the same
    hyper-parameters, parameters and buffers."""
    from collections import OrderedDict
    from oracle import digests as D
    from dpft_amd.configs import load_config
    from dpft_amd.models import build, load
    cfg = load_config("kradar")
    cfg["model"]["backbones"]["camera_mono"]["name"] = "ResNet50"         # keep the CPU test light
    cfg["model"]["fuser"]["dropout"] = 0.05
    comp, m = cfg["computing"], cfg["model"]
    torch.manual_seed(12)
    ours = build("dprt", cfg)                                               # source of the tensors
    with torch.no_grad():
        for p in ours.parameters():
            p.add_(torch.randn_like(p) * 0.01)
    sd = ours.state_dict()
    classes = _ForeignClasses()
    ref = _as_reference_tree(ours, classes, skip=("backbones", "necks")).eval()
    assert D.module_tree_digest(ref, skip=("backbones", "necks")) == golden_digests["dprt_tree"]
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
    assert b"dprt.models.fusers.mpfusion" in ckpt.read_bytes() and b"torchvision.models.resnet" in ckpt.read_bytes()
    model, epoch, stamp = load(str(ckpt))
    assert (epoch, stamp) == (42, "20240101-120000")
    assert type(model).__module__.startswith("dpft_amd.") and not model.training
    got = model.state_dict()
    assert list(got.keys()) == list(sd.keys())
    for k in sd:
        assert torch.equal(got[k], sd[k]), k
    assert model.fuser.dropout == 0.05 and model.fuser.i_iter == 4 and model.inputs == m["inputs"]
    from dpft_amd.models.checkpoint import infer_config, read_foreign
    inferred = infer_config(read_foreign(str(ckpt)))["model"]
    def covers(got, want, path):          # every key of the config with its value; extra inferred keys are checked below
        if isinstance(want, dict):
            for k, v in want.items():
                assert k in got, (path, k)
                covers(got[k], v, path + "." + k)
        else:
            assert got == want, (path, got, want)
    for section in ("inputs", "skiplinks", "backbones", "necks", "embeddings", "querent", "fuser", "head"):
        covers(inferred[section], m[section], section)
    # hyper-parameters that are not tensors are READ from the pickled modules, here the reference's defaults
    e0 = inferred["embeddings"][m["inputs"][0]]
    assert (e0["temperature"], e0["eps"], e0["offset"]) == (10000, 1e-6, 0.0) and abs(e0["scale"] - 6.283185307179586) < 1e-12
    assert inferred["querent"]["distribution"] == ["linear"] * 3 and inferred["fuser"]["ffn_layer"] == "Linear"
    assert inferred["head"]["bias"] is False and inferred["head"]["dropout"] == 0.0
    # ... and a non-default value survives the round trip instead of being replaced by a default
    foreign = read_foreign(str(ckpt))
    for layer in foreign.embeddings[m["inputs"][0]].embedding_layers.values():
        layer.__dict__["temperature"] = 20
    assert infer_config(foreign)["model"]["embeddings"][m["inputs"][0]]["temperature"] == 20
    del foreign.head.__dict__["dropout"]
    with pytest.raises(ValueError, match="dropout"):
        infer_config(foreign)
    # this package's own whole-module checkpoints keep working
    own = tmp_path / "20240101-130000_checkpoint_0001.pt"
    torch.save(ours, str(own))
    again, e2, _ = load(str(own))
    assert e2 == 1 and type(again) is type(ours)


def test_unpickler_does_not_replace_missing_native_classes(tmp_path):
    """Only FOREIGN roots (dprt, torchvision, ...) become stand-ins; a missing class of this package or of torch raises."""
    import pickle
    from dpft_amd.models.checkpoint import ForeignModule, _Unpickler
    import io
    with pytest.raises((AttributeError, ImportError)):
        _Unpickler(io.BytesIO(b"")).find_class("dpft_amd.models.dprt", "NoSuchClass")
    with pytest.raises((AttributeError, ImportError)):
        _Unpickler(io.BytesIO(b"")).find_class("torch.nn", "NoSuchLayer")
    assert issubclass(_Unpickler(io.BytesIO(b"")).find_class("torchvision.models.resnet", "ResNet"), ForeignModule)


def test_whole_module_pickle_drops_process_local_state():
    """``torch.save(model)`` of a model that has run on the GPU (trainer.py:256-258): the HIP streams, the captured decoder
    graphs and the fused inference decoder parked in ``__dict__`` must not reach the pickle (a ``torch.Stream`` cannot be
    pickled at all), nor the trainer's reducer links or device-side table caches.  The GPU round trip is
    tests/test_gpu_trainer.py; this is the mechanism, on the CPU."""
    import io
    from dpft_amd.configs import load_config
    from dpft_amd.models import build
    from dpft_amd.training.trainer import DataParallelTrainer
    cfg = copy.deepcopy(load_config("kradar"))
    cfg["model"]["backbones"]["camera_mono"]["name"] = "ResNet50"
    model = build("dprt", cfg)
    tr = DataParallelTrainer(model, cfg, "cpu")
    assert model.necks["camera_mono"].grad_direct is tr.reducer
    model.__dict__["_view_streams"] = [torch.Stream(device="cpu")]          # what DPRT._place_streams leaves behind
    model.__dict__["_queues_found"] = 3
    model.__dict__["_graphed_fuser"] = lambda: None                          # unpicklable stand-ins
    model.fuser.__dict__["_fused_decoder"] = lambda: None
    emb = model.embeddings["camera_mono"].embedding_layers["embedding0"]
    emb._tables[(1, 1, "cpu")] = (torch.zeros(1), torch.zeros(1))
    model.querent._cache[("k",)] = torch.zeros(1)
    buf = io.BytesIO()
    torch.save(model, buf)
    buf.seek(0)
    again = torch.load(buf, weights_only=False)
    for k in ("_view_streams", "_queues_found", "_graphed_fuser"):
        assert k not in again.__dict__ and k in model.__dict__          # dropped from the pickle, kept on the live model
    assert "_fused_decoder" not in again.fuser.__dict__
    assert again.necks["camera_mono"].grad_direct is None and again.backbones["radar_bev"].grad_direct is None
    assert again.embeddings["camera_mono"].embedding_layers["embedding0"]._tables == {} and again.querent._cache == {}
    for (k, a), (k2, b) in zip(model.state_dict().items(), again.state_dict().items()):
        assert k == k2 and torch.equal(a, b) and a.stride() == b.stride(), k


def test_scheduler_factory_matches_torch():
    """``build_scheduler`` (src/dprt/training/scheduler.py:30-36): plain, chained and sequential schedules."""
    from dpft_amd.training.scheduler import build_scheduler
    def lrs(spec, n=6):
        p = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.SGD([p], lr=1.0)
        spec = copy.deepcopy(spec)
        sch = build_scheduler(spec.pop("name"), **spec)(opt)
        out = []
        for _ in range(n):
            out.append(opt.param_groups[0]["lr"])
            opt.step()
            sch.step()
        return out
    assert lrs({"name": "ConstantLR", "factor": 1.0}) == [1.0] * 6
    assert lrs({"name": "StepLR", "step_size": 2, "gamma": 0.1})[:5] == pytest.approx([1, 1, 0.1, 0.1, 0.01])
    seq = {"name": "SequentialLR", "milestones": [2],
           "schedulers": [{"name": "ConstantLR", "factor": 0.5, "total_iters": 2}, {"name": "ExponentialLR", "gamma": 0.5}]}
    assert lrs(seq)[:5] == pytest.approx([0.5, 0.5, 1.0, 0.5, 0.25])
    ch = {"name": "ChainedScheduler",
          "schedulers": [{"name": "ExponentialLR", "gamma": 0.5}, {"name": "ConstantLR", "factor": 0.1, "total_iters": 1}]}
    assert lrs(ch)[:3] == pytest.approx([0.1, 0.5, 0.25])
    assert seq["schedulers"][0]["name"] == "ConstantLR"      # the config is not consumed (the reference pops from it)


def test_c_assignment_solver_returns_scipys_pairs_in_scipys_order():
    """dpft_lsap_batch_f32 (host code of the matcher, dpft_amd/csrc/cabi.cpp) vs scipy.optimize.linear_sum_assignment -- the
    call the reference makes per sample (training/loss.py:305): same pairs, same order, on random rectangular problems in both
    orientations, with many and with heavy ties, empty samples, and the -1 padding; non-finite costs are refused."""
    import numpy as np
    from scipy.optimize import linear_sum_assignment
    from dpft_amd.hip.lib import lib
    rng = np.random.default_rng(0)

    def run(cost, counts):
        B, N, Mmax = cost.shape
        match = np.empty((B, Mmax, 2), np.int32)
        nm = np.empty(B, np.int32)
        cnt = np.asarray(counts, np.int32)
        return lib.dpft_lsap_batch_f32(cost.ctypes.data, B, N, Mmax, cnt.ctypes.data, match.ctypes.data, nm.ctypes.data), match, nm

    for trial in range(1200):
        B, N, Mmax = int(rng.integers(1, 5)), int(rng.integers(1, 40)), int(rng.integers(1, 12))
        cost = rng.standard_normal((B, N, Mmax)).astype(np.float32)
        if trial % 4 == 1:
            cost = np.round(cost * 2) / 2
        elif trial % 4 == 2:
            cost = np.abs(cost) * 1e3
        elif trial % 4 == 3:
            cost[:] = rng.integers(0, 3, cost.shape)
        counts = rng.integers(0, Mmax + 1, B)
        rc, match, nm = run(cost, counts)
        assert rc == 0
        for b in range(B):
            m = int(counts[b])
            if m == 0:
                assert nm[b] == 0 and (match[b] == -1).all()
                continue
            i, j = linear_sum_assignment(cost[b, :, :m])
            k = len(i)
            assert nm[b] == k and (match[b, :k, 0] == i).all() and (match[b, :k, 1] == j).all() and (match[b, k:] == -1).all(), (trial, b)
    cost = rng.standard_normal((4, 400, 7)).astype(np.float32)          # the training step's shape
    rc, match, nm = run(cost, [7, 3, 0, 1])
    assert rc == 0 and list(nm) == [7, 3, 0, 1]
    for b, m in enumerate([7, 3, 0, 1]):
        if m:
            i, j = linear_sum_assignment(cost[b, :, :m])
            assert (match[b, :m, 0] == i).all() and (match[b, :m, 1] == j).all()
    cost[1, 5, 2] = np.nan
    assert run(cost, [7, 3, 0, 1])[0] != 0 and b"non-finite" in lib.dpft_last_error()
    cost[1, 5, 2] = 0.0
    cost[3, 7, 6] = np.inf                                               # beyond the sample's count: not looked at
    assert run(cost, [7, 3, 0, 1])[0] == 0


def test_integration_shim_loads_the_library_and_exposes_the_extension_api():
    """integration/MultiScaleDeformableAttention.py: the module name and the two callables the reference imports
    (ms_deform_attn.py:24,32,58), bound to the C-ABI symbols of include/dpft_hip.h (no compute without a GPU)."""
    import importlib.util
    import inspect
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("MultiScaleDeformableAttention",
                                                  os.path.join(root, "integration", "MultiScaleDeformableAttention.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert list(inspect.signature(m.ms_deform_attn_forward).parameters) == [
        "value", "spatial_shapes", "level_start_index", "sampling_loc", "attn_weight", "im2col_step"]
    assert list(inspect.signature(m.ms_deform_attn_backward).parameters) == [
        "value", "spatial_shapes", "level_start_index", "sampling_loc", "attn_weight", "grad_output", "im2col_step"]
    assert m._lib.dpft_msda_fwd_f32 and m._lib.dpft_msda_bwd_f32
    import torch
    with pytest.raises(RuntimeError):      # CPU tensors are refused, not computed on some fallback
        m.ms_deform_attn_forward(torch.zeros(1, 4, 2, 2), torch.tensor([[2, 2]]), torch.tensor([0]),
                                 torch.zeros(1, 3, 2, 1, 1, 2), torch.zeros(1, 3, 2, 1, 1), 64)
