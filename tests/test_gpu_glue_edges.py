"""The small kernels between the decoder's backward and the optimizer (misc.hip, optim.hip) at their tile, table and alignment
edges: dpft_sum_leading_f32, dpft_add_many_f32, dpft_memops, dpft_i64_add_many, dpft_adamw_f32 (through FusedAdamW) and
dpft_match_cost_f32.  Each has a host-built table with a hard maximum, a 16-byte vector path chosen by pointer alignment and a
scalar fallback; the training step reaches them only at the model's own sizes.  Every destination sits between guard words of a
known bit pattern; every refused call must leave its destination untouched.  All entry points are called through
dpft_amd.hip.lib, as dpft_amd.hip.ops and the optimizer do."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
POISON = 0x7FC0DEAD                   # a quiet NaN no arithmetic produces
GUARD = 8                             # guard words on each side (a multiple of 4: keeps 16-byte alignment)
ALIGNS = [(16, 16), (16, 4), (4, 16), (4, 4)]      # (dst, src) pointer alignment in bytes


def _lib():
    from dpft_amd.hip.lib import lib, stream
    return lib, stream


def _err():
    from dpft_amd.hip.lib import HipLibraryError
    return HipLibraryError


class Guarded:
    """``n`` 4-byte words at exactly ``align`` (16, or 4 = 16k + 4 * skew) bytes of alignment inside a poisoned buffer."""

    def __init__(self, n, align=16, skew=1):
        off = GUARD + (0 if align == 16 else skew)
        self.buf = torch.full((off + n + GUARD + 4,), POISON, dtype=torch.int32, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.off, self.n = off, n
        self.words = self.buf[off:off + n]
        self.f32 = self.words.view(torch.float32)
        self.ptr = self.words.data_ptr()
        assert self.ptr % 16 == (0 if align == 16 else 4 * skew)

    def guards_intact(self):
        return bool((self.buf[:self.off] == POISON).all()) and bool((self.buf[self.off + self.n:] == POISON).all())

    def untouched(self):
        return bool((self.buf == POISON).all())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------
# dpft_sum_leading_f32
# ---------------------------------------------------------------------------------------------------------------------
N_LEAD = [1, 2, 3, 4, 5, 7, 8, 9]      # either side of the kernel's unroll by 4, every remainder


def _sum_leading(srcs, inner, dst_ptr, accumulate, n_src=None):
    from dpft_amd.hip.lib import SumSrc
    lib, stream = _lib()
    arr = (SumSrc * len(srcs))(*[SumSrc(p, nl) for p, nl in srcs])
    lib.call("dpft_sum_leading_f32", len(srcs) if n_src is None else n_src, C.cast(arr, C.c_void_p), inner, dst_ptr, int(accumulate),
             stream())


def _sequential_f32(dst0, srcs, accumulate):
    """The documented order in IEEE fp32: dst first when accumulating, sources in table order, leading index ascending."""
    acc = dst0.numpy().copy() if accumulate else np.zeros(dst0.numel(), np.float32)
    for s in srcs:
        a = s.numpy()
        for l in range(a.shape[0]):
            acc = acc + a[l]
            assert acc.dtype == np.float32
    return torch.from_numpy(acc)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("inner", [4, 1020, 1024, 1028])
@pytest.mark.parametrize("n_src", [1, 16])
def test_sum_leading_every_unroll_remainder_bitwise(n_src, inner, accumulate):
    """The kernel only adds, in a documented order: with normal operands the result is bit-identical to a sequential numpy.float32
    sum in that order; with integer operands it is the fp64 sum exactly.  inner on either side of one 256-thread block of float4
    (1024), n_lead on either side of the unroll by 4, 1 and the table maximum of 16 sources.  accumulate = 0 overwrites a
    NaN-poisoned destination: no NaN survives."""
    g = torch.Generator().manual_seed(1000 * n_src + 10 * inner + accumulate)
    leads = [[nl] for nl in N_LEAD] if n_src == 1 else [[N_LEAD[(i + rot) % 8] for i in range(16)] for rot in (0, 3)]
    for lead in leads:
        for integers in (True, False):
            draw = (lambda *s: torch.randint(-8, 9, s, generator=g).float()) if integers else (lambda *s: torch.randn(*s, generator=g))
            srcs = [draw(nl, inner) for nl in lead]
            dst0 = draw(inner)
            dst = Guarded(inner)
            if accumulate:
                dst.f32.copy_(dst0)
            dev = [s.to(DEV) for s in srcs]
            assert all(d.data_ptr() % 16 == 0 for d in dev)
            _sum_leading([(d.data_ptr(), nl) for d, nl in zip(dev, lead)], inner, dst.ptr, accumulate)
            torch.cuda.synchronize()
            got = dst.f32.cpu()
            what = f"n_src {n_src}, n_lead {lead}, inner {inner}, accumulate {accumulate}, integers {integers}"
            assert dst.guards_intact(), what
            assert not torch.isnan(got).any(), what
            if integers:
                ref = sum(s.double().sum(0) for s in srcs) + (dst0.double() if accumulate else 0.0)
                assert torch.equal(got.double(), ref), what
            else:
                assert torch.equal(_bits(got), _bits(_sequential_f32(dst0, srcs, accumulate))), what


def test_sum_leading_refuses_bad_tables_and_alignments():
    inner = 8
    src = torch.ones(2 * inner + 4, dtype=torch.float32, device=DEV)
    ok = (src.data_ptr(), 2)
    cases = {
        "17 sources": dict(srcs=[ok] * 17, inner=inner),
        "0 sources": dict(srcs=[ok], inner=inner, n_src=0),
        "inner 6": dict(srcs=[ok], inner=6),
        "inner 0": dict(srcs=[ok], inner=0),
        "src 4-byte aligned": dict(srcs=[ok, (src.data_ptr() + 4, 2)], inner=inner),
        "null src": dict(srcs=[(None, 2)], inner=inner),
        "n_lead 0": dict(srcs=[(src.data_ptr(), 0)], inner=inner),
    }
    for name, kw in cases.items():
        for acc in (0, 1):
            dst = Guarded(inner)
            with pytest.raises(_err(), match="sum_leading"):
                _sum_leading(kw["srcs"], kw["inner"], dst.ptr, acc, kw.get("n_src"))
            torch.cuda.synchronize()
            assert dst.untouched(), name
    dst = Guarded(inner, align=4)
    with pytest.raises(_err(), match="sum_leading"):
        _sum_leading([ok], inner, dst.ptr, 0)
    torch.cuda.synchronize()
    assert dst.untouched(), "dst 4-byte aligned"
    dst = Guarded(inner)                                                 # the same source is accepted with valid arguments
    _sum_leading([ok] * 16, inner, dst.ptr, 0)
    assert torch.equal(dst.f32, torch.full((inner,), 32.0, device=DEV)) and dst.guards_intact()


# ---------------------------------------------------------------------------------------------------------------------
# dpft_add_many_f32
# ---------------------------------------------------------------------------------------------------------------------
def test_add_many_every_tail_and_alignment_pair_bitwise():
    """One launch over 32 entries: n on either side of the float4 width and of one 256-thread pass of float4 (1024), each with
    the four (dst, src) alignment pairs -- vector body + scalar tail, or the scalar loop.  Bit-exact against fp32 a + b."""
    lib, stream = _lib()
    g = torch.Generator().manual_seed(21)
    entries = []
    for n in (1, 3, 4, 5, 1023, 1024, 1025, 4099):
        for k, (ad, as_) in enumerate(ALIGNS):
            a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
            d, s = Guarded(n, ad, skew=1 + k % 3), Guarded(n, as_, skew=3 - k % 3)
            d.f32.copy_(a)
            s.f32.copy_(b)
            entries.append((n, ad, as_, a, b, d, s))
    table = torch.tensor([(d.ptr, s.ptr, 4 * n) for n, _, _, _, _, d, s in entries], dtype=torch.int64).to(DEV)
    lib.call("dpft_add_many_f32", len(entries), table.data_ptr(), stream())
    torch.cuda.synchronize()
    for n, ad, as_, a, b, d, s in entries:
        what = f"n {n}, dst align {ad}, src align {as_}"
        assert torch.equal(_bits(d.f32), _bits(a + b)), what
        assert d.guards_intact() and s.guards_intact() and torch.equal(_bits(s.f32), _bits(b)), what
    with pytest.raises(_err(), match="add_many"):
        lib.call("dpft_add_many_f32", 0, table.data_ptr(), stream())
    with pytest.raises(_err(), match="add_many"):
        lib.call("dpft_add_many_f32", 1, None, stream())


# ---------------------------------------------------------------------------------------------------------------------
# dpft_memops
# ---------------------------------------------------------------------------------------------------------------------
BLOCK_BYTES = 256 * 16 * 8            # MEMOP_BLOCK_BYTES: what one block moves in one pass
GRID_CAP = 2048                       # blocks per operation
MEMOP_BYTES = [4, 12, 16, 20, 28, BLOCK_BYTES, BLOCK_BYTES + 4, GRID_CAP * BLOCK_BYTES + 20]


def _memops(ops, n=None):
    from dpft_amd.hip.lib import MemOp
    lib, stream = _lib()
    arr = (MemOp * len(ops))(*[MemOp(d, s, b) for d, s, b in ops])
    lib.call("dpft_memops", len(ops) if n is None else n, C.cast(arr, C.c_void_p), stream())


_memop_src = {}


def _source_words(n):
    """Random non-zero, non-poison words on the device, 16 spare words behind them; shared by the cases of one size."""
    if n not in _memop_src:
        g = torch.Generator(device=DEV).manual_seed(31)
        _memop_src[n] = torch.randint(1, 2 ** 30, (n + 16,), dtype=torch.int32, device=DEV, generator=g)
    return _memop_src[n]


@pytest.mark.parametrize("fill", [False, True], ids=["copy", "zero-fill"])
@pytest.mark.parametrize("nbytes", MEMOP_BYTES)
def test_memops_every_tail_alignment_pair_and_the_grid_cap(nbytes, fill):
    """Sizes on either side of the 16-byte width, of one block's 32768 bytes and -- 2048 * 32768 + 20 bytes: one block's worth
    past the grid cap plus a one-word tail -- where the grid-stride loop actually loops.  Each with the four (dst, src)
    alignment pairs, as a copy and as a zero fill, between guard words."""
    n = nbytes // 4
    src = _source_words(n)
    for k, (ad, as_) in enumerate(ALIGNS):
        s = src[0:n] if as_ == 16 else src[1 + k % 3:1 + k % 3 + n]
        assert s.data_ptr() % 16 == (0 if as_ == 16 else 4 * (1 + k % 3))
        d = Guarded(n, ad, skew=3 - k % 3)
        _memops([(d.ptr, None if fill else s.data_ptr(), nbytes)])
        torch.cuda.synchronize()
        what = f"{nbytes} bytes, dst align {ad}, src align {as_}, fill {fill}"
        assert d.guards_intact(), what
        if fill:
            assert not bool(d.words.any()), what
        else:
            assert torch.equal(d.words, s), what
        del d


def test_memops_sixteen_operations_in_one_call_and_the_refusals():
    sizes = [4, 12, 16, 20, 28, BLOCK_BYTES, BLOCK_BYTES + 4, 3 * BLOCK_BYTES + 36]
    src = _source_words(4 * BLOCK_BYTES // 4)
    ops, dsts = [], []
    for i in range(16):
        nb = sizes[i % 8]
        ad, as_ = ALIGNS[(i // 2) % 4]
        fill = i % 2 == 1
        d = Guarded(nb // 4, ad)
        s = src[(0 if as_ == 16 else 3) + 4 * i:][:nb // 4]
        ops.append((d.ptr, None if fill else s.data_ptr(), nb))
        dsts.append((d, s, fill))
    _memops(ops)
    torch.cuda.synchronize()
    for i, (d, s, fill) in enumerate(dsts):
        assert d.guards_intact(), i
        assert (not bool(d.words.any())) if fill else torch.equal(d.words, s), i
    # refusals: nothing is launched, no destination is written
    fresh = [Guarded(8) for _ in range(17)]
    good = [(d.ptr, src.data_ptr(), 32) for d in fresh]
    bad = {
        "17 operations": (good, None),
        "0 operations": (good[:1], 0),
        "size not a multiple of 4": (good[:3] + [(fresh[3].ptr, src.data_ptr(), 6)], None),
        "null dst": (good[:2] + [(None, src.data_ptr(), 32)], None),
        "2-byte aligned dst": ([(fresh[0].ptr + 2, src.data_ptr(), 8)], None),
    }
    for name, (ops, n) in bad.items():
        with pytest.raises(_err(), match="memops"):
            _memops(ops, n)
        torch.cuda.synchronize()
        assert all(d.untouched() for d in fresh), name
    lib, stream = _lib()
    with pytest.raises(_err(), match="memops"):
        lib.call("dpft_memops", 1, None, stream())


# ---------------------------------------------------------------------------------------------------------------------
# dpft_i64_add_many
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64, 65, 256, 257])
def test_i64_add_many_block_edges_table_limit_and_a_negative_increment(n):
    """n on either side of the 64-thread block and at the table maximum (256; 257 is refused and writes nothing); an increment of
    -3 on values near 2^40 (both halves of the 64-bit word matter)."""
    lib, stream = _lib()
    base = (1 << 40) + torch.arange(264, dtype=torch.int64) * ((1 << 31) + 7) - 100
    t = base.to(DEV)
    arr = (C.c_void_p * n)(*[t.data_ptr() + 8 * (i + 4) for i in range(n)])
    if n > 256:
        with pytest.raises(_err(), match="i64_add_many"):
            lib.call("dpft_i64_add_many", n, C.cast(arr, C.c_void_p), -3, stream())
        with pytest.raises(_err(), match="i64_add_many"):
            lib.call("dpft_i64_add_many", 0, C.cast(arr, C.c_void_p), -3, stream())
        arr[0] = t.data_ptr() + 4                                            # 4-byte aligned pointer
        with pytest.raises(_err(), match="i64_add_many"):
            lib.call("dpft_i64_add_many", 1, C.cast(arr, C.c_void_p), -3, stream())
        torch.cuda.synchronize()
        assert torch.equal(t.cpu(), base)
        return
    lib.call("dpft_i64_add_many", n, C.cast(arr, C.c_void_p), -3, stream())
    torch.cuda.synchronize()
    want = base.clone()
    want[4:4 + n] -= 3
    assert torch.equal(t.cpu(), want)


# ---------------------------------------------------------------------------------------------------------------------
# dpft_adamw_f32 through FusedAdamW
# ---------------------------------------------------------------------------------------------------------------------
ADAM_NUMELS = [3, 16384, 5, 16385, 1, 16383, 4, 32775]      # moment offsets 0, 3, 16387, 16392, 32777, 32778, 49161, 49165
U = 2.0 ** -24
U1 = U / (1 - 16 * U)                 # absorbs the second-order terms of the 14 roundings of one update


def _f32(x):
    return float(np.float32(x))


def test_fused_adamw_chunk_edges_and_alignments_vs_fp64_recurrence():
    """Three steps of one parameter group whose tensors end on, one short of and one past a CHUNK = 16384 boundary (and 2 chunks
    + 7), with moment offsets of every residue mod 4 and one parameter that is a view at storage offset 1 (p 4-byte aligned only),
    element by element for p, m and v against the AdamW recurrence in fp64 from the same fp32 inputs, with the entry point's own
    fp32-rounded scalars (decay, step_size, inv_sqrt_bc2, 1 - beta).  Some gradient elements are exactly 0.

    Bound: a running first-order error analysis of adamw_kernel's 14 fp32 roundings per element and step, u = 2^-24 each
    (u / (1 - 16 u) to cover the products of roundings), carried through the three steps alongside the fp64 values:
      m' = m + (g - m) c1              3 roundings (sub, mul, add)    E_m' = (1 - c1) E_m + u (2 |c1 (g - m)| + |m'|)
      v' = v b2 + (c2 g) g             4 (mul, mul, mul, add)         E_v' = b2 E_v + u (|v b2| + 2 |c2 g g| + |v'|)
      s  = sqrt(v')                    1                              E_s  = E_v' / (2 s) + u s          (0 where v' = 0)
      d  = s k + eps                   2 (mul, add)                   E_d  = k E_s + u (|s k| + |d|)
      q  = m' / d                      1                              E_q  = E_m' / d + |m'| E_d / d^2 + u |q|
      p' = p decay - step q            3 (mul, mul, sub)              E_p' = decay E_p + step E_q + u (|p decay| + |step q| + |p'|)
    A contraction of a multiply-add into one fma removes a rounding, never adds one.  The bound on p is asserted to lie below
    the rtol 1e-5 + 1e-6 max|p| of the comparison with torch.optim.AdamW (test_fused_adamw_matches_torch) for every element."""
    from dpft_amd.training.optimizer import CHUNK, FusedAdamW
    assert CHUNK == 16384
    lr, b1, b2, eps, wd, steps = 1e-2, 0.9, 0.999, 1e-8, 1e-2, 3
    g = torch.Generator().manual_seed(41)
    offs = np.cumsum([0] + ADAM_NUMELS[:-1])
    assert {int(o) % 4 for o in offs} == {0, 1, 2, 3}
    assert {int(o) % 4 for o, n in zip(offs, ADAM_NUMELS) if n >= 16383} == {0, 1, 2, 3}      # tensors with a vector body
    params, p0 = [], []
    for n in ADAM_NUMELS:
        init = torch.randn(n, generator=g)
        if n == 16385:
            store = torch.empty(n + 1, device=DEV)
            p = torch.nn.Parameter(store[1:])                                    # storage offset 1
            assert p.data_ptr() % 16 == 4
        else:
            p = torch.nn.Parameter(torch.empty(n, device=DEV))
            assert p.data_ptr() % 16 == 0
        p.data.copy_(init)
        params.append(p)
        p0.append(init)
    opt = FusedAdamW(params, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    # the entry point's scalars: fp32 arguments, fp64 arithmetic, fp32 results (dpft_adamw_f32)
    lr32, b1_32, b2_32, eps32, wd32 = _f32(lr), _f32(b1), _f32(b2), _f32(eps), _f32(wd)
    decay = _f32(1.0 - lr32 * wd32)
    c1, c2 = _f32(np.float32(1) - np.float32(b1)), _f32(np.float32(1) - np.float32(b2))
    P = [t.double().numpy() for t in p0]
    M = [np.zeros(n) for n in ADAM_NUMELS]
    V = [np.zeros(n) for n in ADAM_NUMELS]
    EP, EM, EV = ([np.zeros(n) for n in ADAM_NUMELS] for _ in range(3))
    for step in range(1, steps + 1):
        step_size = _f32(lr32 / (1.0 - b1_32 ** step))
        k = _f32(1.0 / np.sqrt(1.0 - b2_32 ** step))
        for i, (p, n) in enumerate(zip(params, ADAM_NUMELS)):
            grad = torch.randn(n, generator=g)
            grad[torch.rand(n, generator=g) < 0.1] = 0.0                          # exact zeros (first step: m = v = 0, q = 0 / eps)
            if n >= 4:
                grad[n - 1] = 0.0
            p.grad = grad.to(DEV)
            assert p.grad.data_ptr() % 16 == 0
            gd = grad.double().numpy()
            m, v, pp = M[i], V[i], P[i]
            m1 = m + (gd - m) * c1
            em = (1 - c1) * EM[i] + U1 * (2 * np.abs(c1 * (gd - m)) + np.abs(m1))
            v1 = v * b2_32 + c2 * gd * gd
            ev = b2_32 * EV[i] + U1 * (np.abs(v * b2_32) + 2 * np.abs(c2 * gd * gd) + np.abs(v1))
            s = np.sqrt(v1)
            es = np.where(v1 > 0, ev / (2 * np.where(v1 > 0, s, 1.0)), 0.0) + U1 * s
            d = s * k + eps32
            ed = k * es + U1 * (np.abs(s * k) + np.abs(d))
            q = m1 / d
            eq = em / d + np.abs(m1) * ed / d ** 2 + U1 * np.abs(q)
            p1 = pp * decay - step_size * q
            ep = decay * EP[i] + step_size * eq + U1 * (np.abs(pp * decay) + np.abs(step_size * q) + np.abs(p1))
            M[i], V[i], P[i], EM[i], EV[i], EP[i] = m1, v1, p1, em, ev, ep
        opt.step()
    torch.cuda.synchronize()
    for i, (p, n) in enumerate(zip(params, ADAM_NUMELS)):
        st = opt.state[p]
        pmax = float(np.abs(P[i]).max())
        assert (EP[i] < 1e-5 * np.abs(P[i]) + 1e-6 * pmax).all(), f"numel {n}: the derived bound is not tighter than the torch comparison"
        for name, got, ref, err in (("p", p.data, P[i], EP[i]), ("m", st["exp_avg"], M[i], EM[i]), ("v", st["exp_avg_sq"], V[i], EV[i])):
            got = got.detach().cpu().double().numpy().reshape(-1)
            diff = np.abs(got - ref)
            w = int(np.argmax(diff - err))
            print(f"adamw numel {n} {name}: max |diff| / bound = {float((diff / np.maximum(err, 1e-300)).max()):.3f}")
            assert (diff <= err).all(), (f"numel {n} (moment offset {int(offs[i])}), {name}: {int((diff > err).sum())} elements above "
                                         f"the bound; worst at {w}: |{got[w]!r} - {ref[w]!r}| = {diff[w]:.3e} > {err[w]:.3e}")


# ---------------------------------------------------------------------------------------------------------------------
# dpft_match_cost_f32
# ---------------------------------------------------------------------------------------------------------------------
MC_B, MC_N, MC_M, MC_C = 2, 37, 5, 3
MC_COUNTS = (5, 2)
MC_WEIGHTS = (1.0, 2.0, 1.5, 0.5, 2.0)      # class, center, size, angle, giou


def match_cost_inputs():
    """Predictions and padded targets (fp32, CPU).  Prediction (0, 3) is degenerate (size 0), prediction (0, 7) is target (0, 2)
    itself, a third of the predictions sit near a target (overlapping boxes), the rest are far (GIoU from the enclosing box)."""
    g = torch.Generator().manual_seed(51)
    B, N, M, Cc = MC_B, MC_N, MC_M, MC_C
    gt_center = torch.randn(B, M, 3, generator=g) * 6
    gt_size = torch.rand(B, M, 3, generator=g) * 3 + 1
    gt_angle = torch.randn(B, M, 2, generator=g)
    gt_id = torch.randint(0, Cc, (B, M), generator=g).int()
    cls = torch.randn(B, N, Cc, generator=g)
    center = torch.randn(B, N, 3, generator=g) * 6
    size = torch.rand(B, N, 3, generator=g) * 3 + 0.5
    angle = torch.randn(B, N, 2, generator=g)
    for b in range(B):
        for i in range(0, N, 3):
            j = (i // 3) % MC_COUNTS[b]
            center[b, i] = gt_center[b, j] + torch.randn(3, generator=g) * 0.5
    size[0, 3] = 0.0
    center[0, 7], size[0, 7], angle[0, 7] = gt_center[0, 2], gt_size[0, 2], gt_angle[0, 2]
    return dict(cls=cls, center=center, size=size, angle=angle, gt_center=gt_center, gt_size=gt_size, gt_angle=gt_angle, gt_id=gt_id)


def oracle_cost(t, dtype):
    """The matcher cost of oracle.dprt_oracle.hungarian (class term, three L1 terms, GIoU3D of yaw boxes) for the rows below
    counts[b], evaluated in ``dtype`` from the same fp32 inputs; 0 elsewhere.  Returned as fp64."""
    from oracle import dprt_oracle as O
    w = MC_WEIGHTS
    out = torch.zeros(MC_B, MC_N, MC_M, dtype=torch.float64)
    for b, m in enumerate(MC_COUNTS):
        cls, ce, sz, an = (t[k][b].to(dtype) for k in ("cls", "center", "size", "angle"))
        gc, gs, ga = (t[k][b, :m].to(dtype) for k in ("gt_center", "gt_size", "gt_angle"))
        cost_class = -cls[:, t["gt_id"][b, :m].long()]
        l1 = lambda x, y: (x[:, None, :] - y[None, :, :]).abs().sum(-1)
        yaw_p, yaw_g = torch.atan2(an[:, 0], an[:, 1]), torch.atan2(ga[:, 0], ga[:, 1])
        giou = O.giou3d_yaw(ce, sz, yaw_p, gc, gs, yaw_g)
        c = w[0] * cost_class + w[1] * l1(ce, gc) + w[2] * l1(sz, gs) + w[3] * l1(an, ga) + w[4] * (-giou.to(dtype))
        assert c.dtype == dtype
        out[b, :, :m] = c.double()
    return out


def test_match_cost_values_vs_fp64_oracle():
    """The values of match_cost_kernel (only the Hungarian indices computed from them were compared so far) against the fp64
    oracle cost; columns j >= counts[b] are exactly 0 (the padded target rows hold NaN: they must not be read).

    Tolerance, measured and not fitted to the kernel: the same oracle formula with every tensor cast to fp32 on the CPU lies at
    most 1.026e-05 from its fp64 value over these inputs (max |cost| 96.4); 4 times that distance, 4.104e-05, is allowed -- the
    kernel's atan2f and fp32 L1 sums are a different but equally rounded evaluation.  Both figures are recomputed here."""
    lib, stream = _lib()
    t = match_cost_inputs()
    ref = oracle_cost(t, torch.float64)
    dist = float((oracle_cost(t, torch.float32) - ref).abs().max())
    tol = 4 * dist
    print(f"match_cost: fp32 oracle vs fp64 oracle max distance {dist:.3e}, tolerance {tol:.3e}, max |cost| {float(ref.abs().max()):.3f}")
    assert 0 < dist < 1e-4
    gt_box = torch.full((MC_B, MC_M, 8), float("nan"))
    for b, m in enumerate(MC_COUNTS):
        gt_box[b, :m] = torch.cat((t["gt_center"][b, :m], t["gt_size"][b, :m], t["gt_angle"][b, :m]), -1)
    dev = {k: t[k].contiguous().to(DEV) for k in ("cls", "center", "size", "angle", "gt_id")}
    gt_box_d = gt_box.to(DEV)
    counts = torch.tensor(MC_COUNTS, dtype=torch.int32, device=DEV)
    cost = Guarded(MC_B * MC_N * MC_M)
    cw = (C.c_float * 5)(*MC_WEIGHTS)
    lib.call("dpft_match_cost_f32", dev["cls"].data_ptr(), dev["center"].data_ptr(), dev["size"].data_ptr(), dev["angle"].data_ptr(),
             gt_box_d.data_ptr(), dev["gt_id"].data_ptr(), counts.data_ptr(), C.byref(cw), cost.ptr, MC_B, MC_N, MC_M, MC_C, stream())
    torch.cuda.synchronize()
    assert cost.guards_intact()
    got = cost.f32.cpu().view(MC_B, MC_N, MC_M)
    for b, m in enumerate(MC_COUNTS):
        assert torch.equal(_bits(got[b, :, m:]), torch.zeros_like(_bits(got[b, :, m:]))), f"sample {b}: padded columns not exactly 0"
    assert not torch.isnan(got).any()
    diff = (got.double() - ref).abs()
    print(f"match_cost: kernel vs fp64 oracle max distance {float(diff.max()):.3e}")
    w = np.unravel_index(int(diff.argmax()), diff.shape)
    assert float(diff.max()) <= tol, f"cost{tuple(int(i) for i in w)}: {float(got[w])!r} vs {float(ref[w])!r}, distance {float(diff.max()):.3e} > {tol:.3e}"
    # the degenerate prediction: GIoU = -1 against every target; the identical pair: IoU = 1, GIoU = volume / enclosing volume
    from oracle import dprt_oracle as O
    yaw = lambda a: torch.atan2(a[..., 0].double(), a[..., 1].double())
    gi = O.giou3d_yaw(t["center"][0, [3, 7]], t["size"][0, [3, 7]], yaw(t["angle"][0, [3, 7]]), t["gt_center"][0], t["gt_size"][0],
                      yaw(t["gt_angle"][0]))
    k = O.box_corners(t["gt_center"][0, 2:3].double(), t["gt_size"][0, 2:3].double(), yaw(t["gt_angle"][0, 2:3]))[0]
    evol = float((k.max(0).values - k.min(0).values).prod())
    assert bool((gi[0] == -1).all()) and abs(float(gi[1, 2]) - float(t["gt_size"][0, 2].double().prod()) / evol) < 1e-12
    assert float(gi[1, 2]) > 0.5 and int(gi[1].argmax()) == 2
