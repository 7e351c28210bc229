"""The typed multi-scale deformable attention operator (dpft_msda_fwd_typed / dpft_msda_bwd_typed, msda_typed.hip) and the doors
that lead to it (ops.msda_fwd / msda_bwd, MSDeformAttnFunction, MSDeformAttn under autocast, the integration shim), element by
element against the project's one fp64 sampling rule on the lattice of tests/sampler_lattice.py.

Reference: oracle.dprt_oracle.msda_core_floor in float64 on the UPCAST inputs (the 16-bit tensors the kernel reads, widened
exactly) and its autograd (torch ops; never the kernel).  `e32` = the same oracle in float32 on the CPU on the same inputs.

Gates, all derived: with u = 0 (fp32), 2^-11 (half), 2^-8 (bf16) -- half a unit in the last place of the storage type, what ONE
rounding to nearest costs -- and E32(r) the project's fp32 gate for the quantity (forward: 1e-5 max|ref| + 1e-4 |r|; gradients:
max(4 e32, 1e-5 max|ref|) + 1e-4 |r|, tests/test_gpu_sampler_edges.py), a result g passes iff

    |g - r| <= E32(r) + u (|r| + E32(r)) + s,      s = 2^-25 for half (half of its subnormal step 2^-24), else 0:

an fp32-grade result x (|x - r| <= E32) rounded once to the storage type moves by at most u |x| <= u (|r| + E32), or by s where
the type has no more bits.  Inputs are O(1) -- value, grad_out ~ N(0, 1) and attn = rand + 0.25, rounded to the storage type --
so no half overflows.  Every figure is printed before it is asserted (run with -s)."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import sampler_lattice as SL
from tests.test_gpu_sampler_edges import _lsi

pytestmark = pytest.mark.gpu
DEV = "cuda"
TYPES = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}
UNIT = {0: 0.0, 1: 2.0 ** -11, 2: 2.0 ** -8}
SUB = {0: 0.0, 1: 2.0 ** -25, 2: 0.0}
NAMES = {0: "fp32", 1: "half", 2: "bf16"}
CAP = 1023.5            # what replaces +-2^20 pixels where the locations themselves are 16-bit (see _lattice)


def typed_close(got, ref64, dtype, what, ref32=None, where=None):
    """The gate of the module docstring; ``ref32`` given = a gradient (atol from the fp32 oracle's own error), None = forward."""
    ref64 = ref64.detach().double().cpu()
    floor = 1e-5 * max(float(ref64.abs().max()), 1e-6)
    e32 = None if ref32 is None else float((ref32.detach().double().cpu() - ref64).abs().max())
    atol = floor if e32 is None else max(4 * e32, floor)
    u, s = UNIT[dtype], SUB[dtype]
    got_, ref_ = got.detach().double().cpu(), ref64
    assert got_.shape == ref_.shape, (got_.shape, ref_.shape)
    assert torch.isfinite(got_).all(), f"{what}: non-finite result"
    E32 = atol + 1e-4 * ref_.abs()
    gate = E32 + u * (ref_.abs() + E32) + s
    excess = (got_ - ref_).abs() - gate
    i = int(excess.argmax())
    idx = tuple(int(v) for v in np.unravel_index(i, ref_.shape)) if ref_.dim() else ()
    err = float((got_ - ref_).abs().max())
    print(f"{what:52s} max|hip - fp64| {err:.3e}   " + (f"max|fp32 oracle - fp64| {e32:.3e}   " if e32 is not None else "") +
          f"gate atol {atol:.3e} + 1e-4 rel, u {u:.3e}, s {s:.1e}   worst excess {float(excess.max()):.3e}")
    assert float(excess.max()) <= 0, (f"{what}: worst element {idx}: got {float(got_[idx])!r} ref {float(ref_[idx])!r} "
                                      f"gate {float(gate[idx])!r}" + (where(idx) if where else ""))


def _oracle(shapes, value, loc, attn, go):
    """-> ((out, gv, gl, ga) in float64, the same in float32) on the tensors as given (upcast exactly).  The float32 oracle runs
    on the CPU (its error is the yardstick `e32`, as in tests/test_gpu_sampler_edges.py); the float64 one runs the same torch code
    on the GPU, where the widest lattice case (8 heads x 32 channels, 2.3 million samples) takes a fraction of the CPU's 7 s."""
    from oracle import dprt_oracle as O

    def run(dt, dev):
        v, l, a = (x.detach().to(dev).to(dt).requires_grad_(True) for x in (value, loc, attn))
        out = O.msda_core_floor(v, shapes, l, a)
        return tuple(x.detach().cpu() for x in (out,) + torch.autograd.grad(out, (v, l, a), go.detach().to(dev).to(dt)))
    return run(torch.float64, DEV), run(torch.float32, "cpu")


def _typed(value, shapes, loc, attn, go):
    """The typed entries on the tensors as given (their dtypes select dtype / loc32) -> out, gv, gl, ga."""
    from dpft_amd.hip import ops
    sh_t = torch.tensor(shapes, dtype=torch.int64, device=DEV)
    lsi_t = torch.tensor(_lsi(shapes), dtype=torch.int64, device=DEV)
    args = (value.to(DEV), sh_t, lsi_t, loc.to(DEV), attn.to(DEV))
    out = ops.msda_fwd_typed(*args)
    gv, gl, ga = ops.msda_bwd_typed(*args, go.to(DEV))
    T = value.dtype
    assert out.dtype == T and gv.dtype == T and ga.dtype == T and gl.dtype == loc.dtype
    assert out.shape == go.shape and gv.shape == value.shape and gl.shape == loc.shape and ga.shape == attn.shape
    return out, gv, gl, ga


def _check_all(res, r64, r32, dtype, tag, at=None):
    typed_close(res[0], r64[0], dtype, f"{tag} out")
    typed_close(res[1], r64[1], dtype, f"{tag} grad_value", r32[1])
    typed_close(res[2], r64[2], dtype if res[2].dtype != torch.float32 else 0, f"{tag} grad_loc", r32[2], at)
    typed_close(res[3], r64[3], dtype, f"{tag} grad_attn", r32[3], at)


@functools.lru_cache(maxsize=None)
def _lattice(M, P, capped):
    """The full lattice of the power-of-two pyramid.  ``capped``: the locations travel in 16 bits, where +-2^20 pixels do not
    fit beside the half-pixel; those entries become t = 1023.5 / -1024.5.  Then (asserted) the locations are the same bits
    after rounding to float16 and to bfloat16, the kernel's own float32 arithmetic on them gives the intended t exactly, and the
    coverage holds with 1023.5 as "far": the cap on dropped lattice points is 0."""
    shapes = SL.POW2_SHAPES
    t = SL.lattice_t(shapes, M, P, True)
    if capped:
        t = np.where(t >= SL.FAR, CAP, np.where(t <= -SL.FAR, -CAP - 1.0, t))
    loc32 = SL.direct_loc(t, shapes)
    assert np.isfinite(loc32).all()
    l_t = torch.from_numpy(loc32)
    if capped:
        assert torch.equal(l_t.half().float(), l_t), "the capped lattice is not exact in float16"
        assert torch.equal(l_t.bfloat16().float(), l_t), "the capped lattice is not exact in bfloat16"
    assert np.array_equal(SL.replay_direct(loc32, shapes).astype(np.float64), t), "the lattice is not exact in float32"
    SL.assert_coverage(t, shapes, True, far=CAP if capped else SL.FAR, what="capped" if capped else "full")
    loc = torch.stack((l_t, l_t.roll(1, 0)))                                             # N = 2: the batch stride
    return t, np.stack((t, np.roll(t, 1, 0))), loc


def _inputs(seed, shapes, Q, M, D, P, T, N=2):
    g = torch.Generator().manual_seed(seed)
    L, S = len(shapes), sum(h * w for h, w in shapes)
    value = torch.randn(N, S, M, D, generator=g).to(T)
    attn = (torch.rand(N, Q, M, L, P, generator=g) + 0.25).to(T)
    go = torch.randn(N, Q, M * D, generator=g).to(T)
    return value, attn, go


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2: the lattice through every path and type (dtype = 0: held to exactly the gates of test_generic_operator_on_the_lattice)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("M,D", [(8, 32), (2, 8), (3, 8), (1, 64), (8, 2), (3, 5), (1, 1)])
@pytest.mark.parametrize("loc32", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_typed_operator_on_the_lattice(dtype, loc32, M, D, P):
    """out, grad_value, grad_loc, grad_attn of the typed entries; (8,32) (2,8) (1,64): the vector forward for every type, (3,8):
    a query of 3 lanes (16-bit) that does not divide the wave, (8,2) (3,5) (1,1): the scalar forward; the backward's head
    groups are 32, 8, 8, 64, 2, 8 (5 used), 1 lanes wide.  loc32 = 0: the locations have the storage type (for dtype 0 that is
    float32 again: the capped lattice in float32).  With u = 0 the gate IS the fp32 operator's."""
    shapes, T = SL.POW2_SHAPES, TYPES[dtype]
    t, tt, loc = _lattice(M, P, not loc32)
    if not loc32:
        loc = loc.to(T)
    value, attn, go = _inputs(100 + 10 * M + P + D, shapes, t.shape[0], M, D, P, T)
    r64, r32 = _oracle(shapes, value, loc, attn, go)
    res = _typed(value, shapes, loc, attn, go)
    tag = f"typed {NAMES[dtype]} loc{'32' if loc32 else 'T'} M{M} D{D} P{P}"
    at = lambda idx: f" at t = {tt[idx[0], idx[1], idx[2], idx[3], idx[4]].tolist()} of level {shapes[idx[3]]}"
    _check_all(res, r64, r32, dtype, tag, at)
    # the rule on t == -1 / t == size: no slope at all, as for the fp32 operator
    edge = torch.from_numpy((tt == -1) | (tt == SL.sizes_wh(shapes)[None, None, None, :, None, :]))
    assert edge.any() and (res[2].cpu()[edge] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3: ragged waves and tails
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pyramid", ["LP24", "LP1"])
@pytest.mark.parametrize("M,D", [(8, 32), (3, 8)])
@pytest.mark.parametrize("Lq", [1, 2, 3, 65, 129])
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_typed_operator_ragged_waves_and_tails(dtype, Lq, M, D, pyramid):
    """Query counts that leave the last wave (forward: 2 queries per wave at (8,32), 21 at (3,8) in 16 bits; backward: 2 / 8 heads
    per wave) partly or almost wholly empty, on the odd pyramid (strides that are no powers of two; fractional parts .25 / .5 /
    .75 only, so rounding cannot move a sample to another cell -- asserted), with L * P = 24 (three levels, eight points) and
    L * P = 1 (one level, one point).  The locations are float32 (loc32 = 1)."""
    shapes, P = (SL.ODD_SHAPES, 8) if pyramid == "LP24" else (SL.ODD_SHAPES[:1], 1)
    T = TYPES[dtype]
    t = SL.lattice_t(shapes, M, P, False)
    start = (37 * Lq) % (t.shape[0] - 2 * Lq)
    t = np.stack((t[start:start + Lq], t[start + Lq:start + 2 * Lq]))                   # N = 2
    loc32 = SL.direct_loc(t.reshape((2 * Lq,) + t.shape[2:]), shapes).reshape(t.shape)
    t32 = SL.replay_direct(loc32.reshape((2 * Lq,) + t.shape[2:]), shapes).astype(np.float64).reshape(t.shape)
    assert np.isfinite(loc32).all() and np.array_equal(np.floor(t32), np.floor(t))
    loc = torch.from_numpy(loc32)
    value, attn, go = _inputs(300 + Lq + M, shapes, Lq, M, D, P, T)
    r64, r32 = _oracle(shapes, value, loc, attn, go)
    res = _typed(value, shapes, loc, attn, go)
    _check_all(res, r64, r32, dtype, f"ragged {NAMES[dtype]} Lq{Lq} M{M} D{D} {pyramid}")


# ---------------------------------------------------------------------------------------------------------------------
# 4: a base that is aligned to its element only
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,D", [(8, 32), (3, 8)])
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_typed_operator_misaligned_base_equals_aligned(dtype, M, D):
    """value / grad_out / out as contiguous views that start one element into a larger buffer (2-byte aligned in 16 bits, 4-byte
    in fp32): the forward leaves its 16-byte form for the element-wise one.  out, grad_loc and grad_attn equal the aligned run
    bit for bit (the same operations in the same order, msda_typed.hip is compiled without contraction for that).  grad_value is
    a sum of fp32 atomics, whose order differs from launch to launch: it is held to the gates (as the replay test does)."""
    from dpft_amd.hip import ops
    from dpft_amd.hip.lib import lib, ptr, stream
    shapes, P, T, Lq = SL.ODD_SHAPES, 4, TYPES[dtype], 67
    t = SL.lattice_t(shapes, M, P, False)[100:100 + 2 * Lq]
    loc = torch.from_numpy(SL.direct_loc(t, shapes)).view(2, Lq, M, len(shapes), P, 2)
    value, attn, go = _inputs(400 + M, shapes, Lq, M, D, P, T)
    r64, r32 = _oracle(shapes, value, loc, attn, go)
    aligned = _typed(value, shapes, loc, attn, go)

    def shifted(x):
        buf = torch.empty(x.numel() + 9, dtype=x.dtype, device=DEV)
        view = buf[1:1 + x.numel()].view(x.shape)
        view.copy_(x)
        assert view.is_contiguous() and view.data_ptr() % 16 == x.element_size()
        return view
    v_s, go_s = shifted(value), shifted(go)
    out_s = shifted(torch.zeros_like(go))
    sh_t = torch.tensor(shapes, dtype=torch.int64, device=DEV)
    lsi_t = torch.tensor(_lsi(shapes), dtype=torch.int64, device=DEV)
    l_d, a_d = loc.to(DEV), attn.to(DEV)
    N, S = value.shape[:2]
    lib.call("dpft_msda_fwd_typed", ptr(v_s), ptr(sh_t), ptr(lsi_t), ptr(l_d), ptr(a_d), ptr(out_s), N, S, M, D, Lq, len(shapes), P,
             dtype, 1, stream())
    gv, gl, ga = ops.msda_bwd_typed(v_s, sh_t, lsi_t, l_d, a_d, go_s)
    tag = f"misaligned {NAMES[dtype]} M{M} D{D}"
    _check_all((out_s, gv, gl, ga), r64, r32, dtype, tag)
    _check_all(aligned, r64, r32, dtype, tag + " (aligned run)")
    assert torch.equal(out_s, aligned[0]), "out differs between the aligned and the misaligned base"
    assert torch.equal(gl, aligned[2]) and torch.equal(ga, aligned[3])


# ---------------------------------------------------------------------------------------------------------------------
# 5: grad_value is rounded once
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [1, 2])
def test_typed_grad_value_is_rounded_once(dtype):
    """Levels (1,1) and (2,2), Lq = 512, M = 8, D = 32, P = 4, every location inside its map: each of the five pixels' grad_value
    elements is the sum of thousands of contributions (2 * 512 * 4 samples per level land on one pixel or on four).  A sum kept
    in 16 bits loses far more than the gate's one rounding; fp32 sums rounded once pass."""
    shapes, M, D, P, Lq, T = [(1, 1), (2, 2)], 8, 32, 4, 512, TYPES[dtype]
    g = torch.Generator().manual_seed(500 + dtype)
    loc = (torch.rand(2, Lq, M, 2, P, 2, generator=g) * 0.5 + 0.25)                      # t in (-0.25, 0.25) / (0, 1): all inside
    value, attn, go = _inputs(510 + dtype, shapes, Lq, M, D, P, T)
    r64, r32 = _oracle(shapes, value, loc, attn, go)
    adds = float((r64[1] != 0).double().mean())
    assert adds == 1.0
    res = _typed(value, shapes, loc, attn, go)
    _check_all(res, r64, r32, dtype, f"many adds {NAMES[dtype]}")


# ---------------------------------------------------------------------------------------------------------------------
# 6: autograd, AMP, graph replay
# ---------------------------------------------------------------------------------------------------------------------
def _amp_inputs(seed, T, M=8, D=32, P=4, Lq=67, capped=False):
    """``capped``: the far-outside entries at +-1024 pixels instead of +-2^20 (locations that travel as float16 must stay finite)."""
    shapes = SL.ODD_SHAPES
    t = SL.lattice_t(shapes, M, P, False)[50:50 + 2 * Lq]
    if capped:      # (this lattice has no kinks: its far entries are -2^20 + 0.5 and 2^20 + 0.5)
        t = np.where(t >= SL.FAR, CAP, np.where(t <= -SL.FAR + 0.5, -CAP - 1.0, t))
    loc = torch.from_numpy(SL.direct_loc(t, shapes)).view(2, Lq, M, len(shapes), P, 2)
    value, attn, go = _inputs(seed, shapes, Lq, M, D, P, T)
    return shapes, value, loc, attn.float(), go


def test_function_returns_gradients_in_the_input_dtypes():
    """MSDeformAttnFunction.apply with bf16 value, fp32 locations and fp32 weights (what autocast hands over; the weights hold
    bf16 values here so that the cast inside is exact and the reference sees what the kernel sees): bf16 out, gradients
    bf16 / fp32 / fp32, all within the gates."""
    from dpft_amd.models.layers.ms_deform_attn import MSDeformAttnFunction
    shapes, value, loc, attn, go = _amp_inputs(600, torch.bfloat16)
    r64, r32 = _oracle(shapes, value, loc, attn, go)
    v, l, a = (x.to(DEV).requires_grad_(True) for x in (value, loc, attn))
    sh_t = torch.tensor(shapes, dtype=torch.int64, device=DEV)
    lsi_t = torch.tensor(_lsi(shapes), dtype=torch.int64, device=DEV)
    out = MSDeformAttnFunction.apply(v, sh_t, lsi_t, l, a, 64)
    assert out.dtype == torch.bfloat16
    gv, gl, ga = torch.autograd.grad(out, (v, l, a), go.to(DEV))
    assert (gv.dtype, gl.dtype, ga.dtype) == (torch.bfloat16, torch.float32, torch.float32)
    typed_close(out, r64[0], 2, "function bf16 out")
    typed_close(gv, r64[1], 2, "function bf16 grad_value", r32[1])
    typed_close(gl, r64[2], 0, "function bf16 grad_loc (fp32)", r32[2])
    typed_close(ga, r64[3], 2, "function bf16 grad_attn (fp32 tensor, bf16 values)", r32[3])


@pytest.mark.parametrize("T", [torch.bfloat16, torch.float16])
def test_module_runs_under_autocast(T):
    from dpft_amd.models.layers.ms_deform_attn import MSDeformAttn
    torch.manual_seed(610)
    shapes = [(6, 5), (3, 4)]
    mod = MSDeformAttn(d_model=64, n_levels=2, n_heads=8, n_points=2).to(DEV)
    S, Lq = sum(h * w for h, w in shapes), 19
    query = torch.randn(2, Lq, 64, device=DEV, requires_grad=True)
    feats = torch.randn(2, S, 64, device=DEV, requires_grad=True)
    refp = torch.rand(2, Lq, 2, 2, device=DEV)
    sh_t = torch.tensor(shapes, dtype=torch.int64, device=DEV)
    lsi_t = torch.tensor(_lsi(shapes), dtype=torch.int64, device=DEV)
    with torch.autocast("cuda", dtype=T):
        out = mod(query, refp, feats, sh_t, lsi_t)
    assert out.dtype == T and out.shape == (2, Lq, 64)
    out.float().square().sum().backward()
    for n, p in mod.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all(), n
    assert float(mod.value_proj.weight.grad.abs().max()) > 0 and float(mod.sampling_offsets.weight.grad.abs().max()) > 0
    assert torch.isfinite(query.grad).all() and torch.isfinite(feats.grad).all()


def test_step_replays_bit_equal_in_a_graph():
    """Forward + backward through MSDeformAttnFunction captured in a torch.cuda.graph after a warm-up: the replay's out, grad_loc
    and grad_attn are the eager run's bits.  grad_value is a sum of fp32 atomics (arrival order): held to the gates instead."""
    from dpft_amd.models.layers.ms_deform_attn import MSDeformAttnFunction
    shapes, value, loc, attn, go = _amp_inputs(620, torch.bfloat16)
    r64, r32 = _oracle(shapes, value, loc, attn, go)
    v, l, a = (x.to(DEV).requires_grad_(True) for x in (value, loc, attn))
    go_d = go.to(DEV)
    sh_t = torch.tensor(shapes, dtype=torch.int64, device=DEV)
    lsi_t = torch.tensor(_lsi(shapes), dtype=torch.int64, device=DEV)

    def step():
        out = MSDeformAttnFunction.apply(v, sh_t, lsi_t, l, a, 64)
        return (out,) + torch.autograd.grad(out, (v, l, a), go_d)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [x.clone() for x in step()]
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(2):
        for x in captured:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured[0], eager[0]), "out"
        assert torch.equal(captured[2], eager[2]) and torch.equal(captured[3], eager[3]), "grad_loc / grad_attn"
        typed_close(captured[1], r64[1], 2, "replayed grad_value", r32[1])
    typed_close(eager[1], r64[1], 2, "eager grad_value", r32[1])


# ---------------------------------------------------------------------------------------------------------------------
# 7: the integration shim
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loc32", [0, 1])
@pytest.mark.parametrize("dtype", [1, 2])
def test_integration_shim_with_16_bit_tensors(dtype, loc32):
    """integration/MultiScaleDeformableAttention.py driven the way the reference drives the extension (an autograd Function around
    ms_deform_attn_forward / ms_deform_attn_backward, as tests/test_gpu_kernels.py does for fp32) with half and bf16 tensors."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("MultiScaleDeformableAttention",
                                                  os.path.join(root, "integration", "MultiScaleDeformableAttention.py"))
    MSDA = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(MSDA)

    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, value, shapes, lsi, loc, attn, im2col_step):
            ctx.im2col_step = im2col_step
            out = MSDA.ms_deform_attn_forward(value, shapes, lsi, loc, attn, ctx.im2col_step)
            ctx.save_for_backward(value, shapes, lsi, loc, attn)
            return out

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad_output):
            value, shapes, lsi, loc, attn = ctx.saved_tensors
            gv, gl, ga = MSDA.ms_deform_attn_backward(value, shapes, lsi, loc, attn, grad_output, ctx.im2col_step)
            return gv, None, None, gl, ga, None
    T = TYPES[dtype]
    shapes, value, loc, attn, go = _amp_inputs(700 + dtype, T, capped=not loc32)
    attn = attn.to(T)
    if not loc32:
        loc = loc.to(T)      # (rounded locations: the reference below reads the same rounded tensor; the odd pyramid has no kinks)
        assert torch.isfinite(loc).all()
    r64, r32 = _oracle(shapes, value, loc, attn, go)
    v, l, a = (x.to(DEV).requires_grad_(True) for x in (value, loc, attn))
    sh_t = torch.as_tensor(shapes, dtype=torch.long, device=DEV)
    lsi_t = torch.cat((sh_t.new_zeros((1,)), sh_t.prod(1).cumsum(0)[:-1]))
    out = Fn.apply(v, sh_t, lsi_t, l, a, 64)
    assert out.dtype == T
    (out.float() * go.to(DEV).float()).sum().backward()
    assert v.grad.dtype == T and a.grad.dtype == T and l.grad.dtype == loc.dtype
    _check_all((out, v.grad, l.grad, a.grad), r64, r32, dtype, f"shim {NAMES[dtype]} loc{'32' if loc32 else 'T'}")
    with pytest.raises(RuntimeError):      # a CPU tensor, a value dtype no kernel stores, locations of another 16-bit type
        MSDA.ms_deform_attn_forward(value, sh_t, lsi_t, l.detach(), a.detach(), 64)
    with pytest.raises(RuntimeError):
        MSDA.ms_deform_attn_forward(v.detach().double(), sh_t, lsi_t, l.detach(), a.detach(), 64)
    other = torch.bfloat16 if T == torch.float16 else torch.float16
    with pytest.raises(RuntimeError):
        MSDA.ms_deform_attn_forward(v.detach(), sh_t, lsi_t, l.detach().to(other), a.detach(), 64)


# ---------------------------------------------------------------------------------------------------------------------
# 8: the door that was open stays as it was
# ---------------------------------------------------------------------------------------------------------------------
def test_fp32_ops_still_go_to_the_f32_entries_bit_for_bit():
    from dpft_amd.hip import ops
    from dpft_amd.hip.lib import lib, ptr, stream
    shapes, value, loc, attn, go = _amp_inputs(800, torch.float32, M=8, D=2)
    sh_t = torch.tensor(shapes, dtype=torch.int64, device=DEV)
    lsi_t = torch.tensor(_lsi(shapes), dtype=torch.int64, device=DEV)
    v, l, a, g = (x.to(DEV) for x in (value, loc, attn, go))
    N, S, M, D = v.shape
    Lq, L, P = l.shape[1], l.shape[3], l.shape[4]
    direct = torch.empty(N, Lq, M * D, device=DEV)
    lib.call("dpft_msda_fwd_f32", ptr(v), ptr(sh_t), ptr(lsi_t), ptr(l), ptr(a), ptr(direct), N, S, M, D, Lq, L, P, stream())
    out = ops.msda_fwd(v, sh_t, lsi_t, l, a)
    assert out.dtype == torch.float32 and torch.equal(out, direct)
    gv, gl, ga = ops.msda_bwd(v, sh_t, lsi_t, l, a, g)
    dgv, dgl, dga = torch.zeros_like(v), torch.empty_like(l), torch.empty_like(a)
    lib.call("dpft_msda_bwd_f32", ptr(v), ptr(sh_t), ptr(lsi_t), ptr(l), ptr(a), ptr(g), ptr(dgv), ptr(dgl), ptr(dga), N, S, M, D,
             Lq, L, P, stream())
    assert torch.equal(gl, dgl) and torch.equal(ga, dga)      # (grad_value: fp32 atomics, order-dependent)
    torch.testing.assert_close(gv, dgv, rtol=1e-5, atol=1e-6)
