"""The native ResNet launch plan (dpft_amd/csrc/resnet_plan.hip through dpft_amd/models/backbones/resnet.py) against the fp64 oracle
over the lattice of tests/plan_lattice.py: shallow bodies whose depths, multi_scale, batch and map sizes reach the plan's buffer and
dy-slot parities, the pending-BatchNorm bookkeeping, the folded bn3 reductions, both identity branches, the row count of every
BatchNorm, odd and even stem / pool sizes, the eval epilogue path, the frozen-BatchNorm path and the three act16 storage forms.
The CPU half (tests/test_plan_lattice.py) shows that the inputs keep every ReLU and max-pool decision away from a flip and that
no case amplifies round-off, so that every output, every running statistic and EVERY parameter gradient is held on its own.

The bound is the project's rule for "a different but equally rounded evaluation": rel-L2 against the fp64 value <= max(floor,
4 e32), e32 = the fp32 CPU evaluation of the same oracle against fp64, recomputed here; floors 1e-5 (outputs, statistics) and 1e-4
(gradients).  bf16 compute: 4 e16, e16 = the fp64 walk with bf16 operands (and bf16 stored tensors for act16 >= 1) against the
plain fp64 walk; gradients per stage as one vector, since ReLU flips cannot be conditioned away at 2^-9.  Both distances are
printed for every case and tensor group.

A tensor with no bf16 product or store in front of it (the stem's statistics: its conv has C = 3 and runs in fp32 in every mode)
has e16 = 0 exactly; it is held to the fp32 rule.

Measured on an MI355X, worst ratio over cases and tensors.  gpu / e32: train outputs and statistics 2.0, train gradients 3.2 (l4-2x1
layer2.0.bn2.weight, 6.4e-5 against 2.0e-5: under the floor), partial cotangents 2.4, frozen outputs 1.1, frozen gradients 2.6,
inference 1.1; the largest distances are 1.0e-5 (a train output of l4-2x1, bound 2.4e-5) and 7.3e-5 (a train gradient of l4-2x1,
bound 1.8e-4).  gpu / e16, act16 0 | 1 | 2: outputs 1.01 | 1.04 | 1.04, gradients per stage 1.07 | 1.20 | 1.20, running statistics
1.06 | 1.19 | 1.18.  No case needed more than the bound; nothing in the plan or its kernels had to change."""
import pytest
import torch

from tests import plan_lattice as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR_OUT, FLOOR_GRAD = 1e-5, 1e-4


def _device_module(c, mode):
    return L.module(c, mode).to(DEV)


def _check(c, what, name, got, ref64, ref32, floor, worst):
    e, e32 = L.rel_l2(got, ref64), L.rel_l2(ref32, ref64)
    worst.append((e / max(e32, 1e-30), e, e32, name))
    assert bool(torch.isfinite(got).all()), (c.name, what, name, "NaN / Inf")
    assert e <= max(floor, 4 * e32), (c.name, what, name, e, e32)


def _summary(c, what, worst):
    ratio, e, e32, name = max(worst)
    above = [w for w in worst if w[1] > 0.25 * FLOOR_OUT]
    print(f"{c.name:9s} {what:28s} {len(worst):3d} tensors  worst gpu/e32 {ratio:6.2f} (gpu {e:.2e} e32 {e32:.2e} {name})"
          f"  largest gpu {max(w[1] for w in worst):.2e}  above a quarter of the floor: {len(above)}")


def _plan_of(bb, c, act16=0):
    plans = list(bb._plans.values())
    assert len(plans) == 1 and plans[0].act16 == act16, [p.act16 for p in plans]
    plan = plans[0]
    assert plan.n_conv == L.n_convs(c) == sum(isinstance(m, torch.nn.Conv2d) for m in bb.modules())
    assert plan.n_bn == len(L.bn_layers(c)) == sum(isinstance(m, torch.nn.BatchNorm2d) for m in bb.modules())
    assert [shape for _, shape in plan.outs] == L.stage_shapes(c)
    return plan


def _check_outputs(c, what, outs, e64, e32, worst):
    assert list(outs.keys()) == [str(i + 1) for i in range(c.multi_scale)]
    assert [tuple(v.shape) for v in outs.values()] == L.stage_shapes(c)
    for k, v in outs.items():
        _check(c, what, "out " + k, v, e64["outs"][k], e32["outs"][k], FLOOR_OUT, worst)


def _check_grads(c, what, bb, g64, g32, worst):
    names = [n for n, _ in bb.named_parameters()]
    assert sorted(names) == sorted(g64)
    assert ("adjustment_layer.weight" in names) == (c.in_ch != 3) and "body.conv1.weight" in names
    for n, p in bb.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, n
        if float(g64[n].norm()) == 0:              # behind the last cotangent: exactly zero
            assert not bool(p.grad.any()), (c.name, what, n)
        else:
            _check(c, what, n, p.grad, g64[n], g32[n], FLOOR_GRAD, worst)


def _backward(bb, outs, c, stages):
    cots = L.cotangents(c)
    bb.zero_grad(set_to_none=True)
    sum((outs[str(li + 1)] * cots[li].to(DEV)).sum() for li in stages).backward()
    torch.cuda.synchronize()


def _buffers(bb):
    return {k: v.detach().clone() for k, v in bb.state_dict().items() if "running" in k or "num_batches" in k}


@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_train_forward_statistics_and_backward(c):
    """Train mode: stage outputs, the running statistics after one and after two forwards against the fp64 recurrence on the
    tapped pre-BatchNorm tensors, num_batches_tracked, the second forward bit-equal to the first, and every parameter gradient."""
    sd, x, e64, e32 = L.cached(c, "train")
    bb = _device_module(c, "train").train()
    xd = x.to(DEV)
    worst = []
    outs = bb(xd)
    _plan_of(bb, c)
    first = {k: v.detach().cpu() for k, v in outs.items()}
    _check_outputs(c, "train", first, e64, e32, worst)
    for steps in (1, 2):
        if steps == 2:
            again = bb(xd)
            assert all(torch.equal(again[k].detach().cpu(), first[k]) for k in first), c.name
            outs = again
        r64 = L.running_stats(c, sd, e64["taps"]["bn_in"], steps)
        r32 = L.running_stats(c, sd, e32["taps"]["bn_in"], steps, torch.float32)
        mods = dict(bb.named_modules())
        assert len(r64) == len(L.bn_layers(c))
        for name, _, M, _ in L.bn_layers(c):
            assert e64["taps"]["bn_in"][name].numel() // e64["taps"]["bn_in"][name].shape[1] == M      # the rows of the reference
            m = mods[name]
            assert int(m.num_batches_tracked) == steps, (c.name, name)
            _check(c, "train", f"{name}.running_mean x{steps}", m.running_mean, r64[name][0], r32[name][0], FLOOR_OUT, worst)
            _check(c, "train", f"{name}.running_var x{steps}", m.running_var, r64[name][1], r32[name][1], FLOOR_OUT, worst)
    _summary(c, "train outputs + statistics", worst)
    worst = []
    _backward(bb, outs, c, L.cot_sets(c)["all"])
    _check_grads(c, "train", bb, e64["grads"]["all"], e32["grads"]["all"], worst)
    _summary(c, "train gradients", worst)


@pytest.mark.parametrize("name,which", [(n, w) for n in L.PARTIAL for w in L.cot_sets(L.by_name(n)) if w != "all"])
def test_cotangents_on_part_of_the_outputs(name, which):
    """A cotangent on the last stage only / on a middle stage only (where there is a single stage the two are one): the
    gradients upstream match the oracle, the parameters of the stages behind the last cotangent get exactly zero."""
    c = L.by_name(name)
    stages, key = L.cot_sets(c)[which], which
    sd, x, e64, e32 = L.cached(c, "train")
    bb = _device_module(c, "train").train()
    outs = bb(x.to(DEV))
    worst = []
    _backward(bb, outs, c, stages)
    _check_grads(c, which, bb, e64["grads"][key], e32["grads"][key], worst)
    zero = [n for n, g in e64["grads"][key].items() if float(g.norm()) == 0]
    assert bool(zero) == (which == "mid" and len(c.depths) > 2)
    _summary(c, f"train gradients, cotangent {which}", worst)


@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_frozen_batchnorm_forward_and_backward(c):
    """eval() with gradients enabled (plan mode 2): outputs and every parameter gradient against the oracle with train = False;
    running buffers and num_batches_tracked bit-identical before and after."""
    sd, x, e64, e32 = L.cached(c, "eval")
    bb = _device_module(c, "eval").eval()
    before = _buffers(bb)
    outs = bb(x.to(DEV))
    _plan_of(bb, c)
    assert all(v.requires_grad for v in outs.values())
    worst = []
    _check_outputs(c, "frozen", outs, e64, e32, worst)
    _summary(c, "frozen outputs", worst)
    worst = []
    _backward(bb, outs, c, L.cot_sets(c)["all"])
    _check_grads(c, "frozen", bb, e64["grads"]["all"], e32["grads"]["all"], worst)
    _summary(c, "frozen gradients", worst)
    after = _buffers(bb)
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before), c.name


@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_inference_forward(c):
    """eval() under no_grad (plan mode 0: BatchNorm, ReLU and the residual add in the conv epilogues): outputs against the oracle
    with train = False, buffers untouched."""
    sd, x, e64, e32 = L.cached(c, "eval")
    bb = _device_module(c, "eval").eval()
    before = _buffers(bb)
    with torch.no_grad():
        outs = bb(x.to(DEV))
    torch.cuda.synchronize()
    _plan_of(bb, c)
    assert not any(v.requires_grad for v in outs.values())
    worst = []
    _check_outputs(c, "inference", outs, e64, e32, worst)
    _summary(c, "inference outputs", worst)
    after = _buffers(bb)
    assert all(torch.equal(before[k], after[k]) for k in before), c.name


@pytest.mark.parametrize("act16", [0, 1, 2])
@pytest.mark.parametrize("name", L.BF16)
def test_bf16_compute_train_step(name, act16, monkeypatch):
    """conv_set_compute("bf16") with fp32 storage, bf16 activations, bf16 activations and weights: stage outputs, running
    statistics after one forward and the parameter gradients per stage within 4 e16 of the fp64 oracle; every gradient finite."""
    from dpft_amd.hip import ops
    from dpft_amd.models.backbones.resnet import BackboneBase
    c = L.by_name(name)
    sd, x, e64, e32 = L.cached(c, "train")
    q64 = L.cached_bf16(c, act16)
    monkeypatch.setattr(BackboneBase, "ACT16_MIN_PIXELS", 0 if act16 else 1 << 60)
    monkeypatch.setenv("DPFT_ACT16", str(max(act16, 1)))
    bb = _device_module(c, "train").train()
    ops.conv_set_compute("bf16")
    try:
        outs = bb(x.to(DEV))
        _plan_of(bb, c, act16)
        _backward(bb, outs, c, L.cot_sets(c)["all"])
        outs = {k: v.detach().cpu() for k, v in outs.items()}
    finally:
        ops.conv_set_compute("fp32")
    rows = []

    def check(what, got, ref, emu, ref32=None):
        e, e16 = L.rel_l2(got, ref), L.rel_l2(emu, ref)
        assert bool(torch.isfinite(got).all()), (name, act16, what)
        if e16 == 0:
            # no bf16 product or store in front of this tensor (the stem's statistics: its conv has C = 3 and stays fp32 in
            # every mode), so the yardstick is exactly 0 and the tensor is held to the fp32 rule instead
            assert what.startswith("body.bn1.running") and ref32 is not None, (name, act16, what)
            e32_ = L.rel_l2(ref32, ref)
            rows.append((0.0, e, e16, what + " (fp32 rule)"))
            assert e <= max(FLOOR_OUT, 4 * e32_), (name, act16, what, e, e32_)
            return
        rows.append((e / e16, e, e16, what))
        assert e <= 4 * e16, (name, act16, what, e, e16)

    try:
        for k, v in outs.items():
            assert tuple(v.shape) == L.stage_shapes(c)[int(k) - 1]
            check("out " + k, v, e64["outs"][k], q64["outs"][k])
        r64, r16 = L.running_stats(c, sd, e64["taps"]["bn_in"], 1), L.running_stats(c, sd, q64["taps"]["bn_in"], 1)
        r32 = L.running_stats(c, sd, e32["taps"]["bn_in"], 1, torch.float32)
        mods = dict(bb.named_modules())
        for bn, _, _, _ in L.bn_layers(c):
            assert int(mods[bn].num_batches_tracked) == 1
            check(bn + ".running_mean", mods[bn].running_mean, r64[bn][0], r16[bn][0], r32[bn][0])
            check(bn + ".running_var", mods[bn].running_var, r64[bn][1], r16[bn][1], r32[bn][1])
        grads = {n: p.grad.detach().double().cpu() for n, p in bb.named_parameters()}
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())
        cat = lambda src, names: torch.cat([src[n].flatten() for n in names])
        for li, names in L.stage_groups(c, list(grads)).items():
            check(f"gradients of stage {li}", cat(grads, names), cat(e64["grads"]["all"], names), cat(q64["grads"]["all"], names))
    finally:
        for ratio, e, e16, what in rows:
            if "running" not in what or ratio > 2:
                print(f"{name:9s} act16 {act16}  {what:34s} gpu {e:.2e}  e16 {e16:.2e}  ratio {ratio:5.2f}")
        stats = [r for r in rows if "running" in r[3]]
        if stats:
            print(f"{name:9s} act16 {act16}  running statistics: worst ratio {max(stats)[0]:5.2f} over {len(stats)} vectors")
