"""GPU half of the BatchNorm pass lattice (tests/bn_lattice.py): runs a case through the storage-typed entries of dpft_amd.hip.ops
and checks every output bit for bit against the fp64 reference, every guard word, and the kernel form the library reports against
the dispatch restatement.  Used in process by tests/test_gpu_bn_passes.py and, with one dispatch switch changed per process, by
tools/bn_lattice_child.py.  Every function raises AssertionError with the case, pass and variant in the message."""
import torch

from tests import bn_lattice as L

DEV = "cuda"
GUARD = 64


class Guarded:
    """A device buffer with GUARD sentinel elements before and after the part a kernel may write, itself filled with a value no
    kernel of the family produces (NaN; 0xA5 for mask bytes), so that an unwritten element fails the comparison."""

    def __init__(self, shape, dtype):
        n = 1
        for s in shape:
            n *= s
        self.fill = 0xA5 if dtype == torch.uint8 else float("nan")
        self.sentinel = 0x5A if dtype == torch.uint8 else -12288.0      # (exact in bf16)
        self.buf = torch.full((n + 2 * GUARD,), self.sentinel, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        self.t.fill_(self.fill)

    def intact(self):
        g = torch.cat([self.buf[:GUARD], self.buf[self.buf.numel() - GUARD:]])
        return bool((g == self.sentinel).all())

    def untouched(self):
        return bool((self.t == self.fill).all()) if self.t.dtype == torch.uint8 else bool(torch.isnan(self.t).all())


def _dev(t, dtype=torch.float32):
    return t.to(dtype).to(DEV).contiguous()


def _same(got, want64, what):
    """Bit equality with the fp64 reference cast to the output's type (the reference is exactly representable: exact_proof)."""
    want = want64.to(got.dtype).to(got.device)
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        idx = bad.nonzero()[0].tolist()
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r want %r" %
                             (what, int(bad.sum()), got.numel(), idx, got[tuple(idx)].item(), want[tuple(idx)].item()))


def _form(ops, want, what):
    got = ops.bn_last_form()
    assert got == want, "%s: the library took form %r, the dispatch restatement says %r" % (what, got, want)


def run_case(c, sw, storages=(False, True)):
    """Exact tier of one (M, K) case: act x 5 variants, reduce x 5 mask sources, apply train / frozen, per storage type."""
    from dpft_amd.hip import ops
    o = L.exact_operands(c)
    train_sums = L.apply_sums_exact(c.M)
    M, K = c.M, c.K
    bnp, rbnp, gamma = _dev(o["bnp"]), _dev(o["rbnp"]), _dev(o["gamma"])
    for bf16 in storages:
        dt = torch.bfloat16 if bf16 else torch.float32
        st = "bf16" if bf16 else "f32"
        y, res, dout = _dev(o["y"], dt), _dev(o["res"], dt), _dev(o["dout"], dt)
        kept = {}
        for i, v in enumerate(L.ACT_VARIANTS):
            what = "%s act %s %s" % (c.name, st, v)
            want = L.ref_act(o["y"], o["bnp"], o["res"] if v["res"] else None, o["rbnp"] if v["rbn"] else None, v["relu"])
            use32, use8 = i in (2, 4), i != 0
            out, out32, m8 = Guarded((M, K), dt), Guarded((M, K), torch.float32), Guarded((M, K // 4), torch.uint8)
            ops.bn_act_any(y, bnp, res if v["res"] else None, rbnp if v["rbn"] else None, v["relu"], out=out.t,
                           out32=out32.t if use32 else None, mask8=m8.t if use8 else None)
            _form(ops, L.elementwise_launch("act", M, K, bf16, sw, out32=use32).form, what)
            _same(out.t, want, what + " out")
            if use32:
                _same(out32.t, want, what + " out32")
            if use8:
                _same(m8.t, L.mask_bytes(want), what + " mask8")
            assert (use32 or out32.untouched()) and (use8 or m8.untouched()), what + ": an optional output that was not given was written"
            assert out.intact() and out32.intact() and m8.intact(), what + ": guard words overwritten"
            if i == 2:
                kept = dict(out=out.t, mask8=m8.t, out64=want)
        masks = dict(none=({}, L.ref_mask("none", o["y"])), mask8=(dict(mask8=kept["mask8"]), kept["out64"] > 0),
                     out=(dict(out=kept["out"]), kept["out64"] > 0), mask_bnp=(dict(mask_bnp=rbnp), L.bn(o["y"], o["rbnp"]) > 0),
                     # the layer's own block, as the launch plan passes it: the fixed-channel form that reuses y - mean
                     mask_self=(dict(mask_bnp=bnp), L.bn(o["y"], o["bnp"]) > 0))
        for name, (kw, mask) in masks.items():
            what = "%s reduce %s mask=%s" % (c.name, st, name)
            sums = Guarded((2, K), torch.float32)
            sums.t.fill_(7.0)                                    # the entry clears them itself
            ops.bn_bwd_reduce_any(y, dout, bnp, sums=sums.t, **kw)
            _form(ops, "generic", what)
            _same(sums.t, L.ref_reduce(o["y"], o["dout"], o["bnp"], mask), what)
            assert sums.intact(), what + ": guard words overwritten"
            for frozen in (False, True):
                if name in ("none", "out") and frozen:
                    continue
                what = "%s apply %s mask=%s frozen=%s" % (c.name, st, name, frozen)
                fed64 = o["sums_in"] if (train_sums or frozen) else torch.zeros_like(o["sums_in"])
                fed = _dev(fed64)
                dy, dgb, zb = Guarded((M, K), dt), Guarded((2, K), torch.float32), Guarded((2 * K + 3,), torch.float32)
                use_z = name != "none"
                ops.bn_bwd_apply_any(y, dout, bnp, gamma, fed, frozen=frozen, dy=dy.t, dgamma=dgb.t[0], dbeta=dgb.t[1],
                                     zero_buf=zb.t if use_z else None, **kw)
                _form(ops, L.elementwise_launch("apply", M, K, bf16, sw).form, what)
                _same(dy.t, L.ref_apply(o["y"], o["dout"], o["bnp"], o["gamma"], fed64, mask, frozen), what + " dy")
                _same(dgb.t, torch.stack([fed64[1], fed64[0]]), what + " dgamma/dbeta")
                assert bool((zb.t == 0).all()) if use_z else zb.untouched(), what + ": zero_buf"
                assert dy.intact() and dgb.intact() and zb.intact(), what + ": guard words overwritten"


def run_pool_case(c, sw):
    from dpft_amd.hip import ops
    o = L.pool_operands(c)
    y, bnp = _dev(o["y"]), _dev(o["bnp"])
    want, _ = L.ref_pool(o["y"], o["bnp"])
    want_dz = L.ref_pool_bwd(o["y"], o["bnp"], o["dout"])
    for dt in (torch.float32, torch.bfloat16):
        what = "%s %s" % (c.name, dt)
        out = Guarded(tuple(want.shape), dt)
        ops.bn_relu_maxpool_any(y, bnp, out=out.t)
        _form(ops, "generic", what + " pool")
        _same(out.t, want, what + " pool")
        dz = Guarded(tuple(o["y"].shape), torch.float32)
        ops.bn_relu_maxpool_bwd_any(y, bnp, _dev(o["dout"], dt), dz=dz.t)
        _form(ops, L.pool_bwd_form(c.H, c.W, c.K, sw), what + " pool backward")
        _same(dz.t, want_dz, what + " pool backward")
        assert out.intact() and dz.intact(), what + ": guard words overwritten"


def run_sums_case(c, sw):
    """dpft_bn_act_sums_f32: y side only, residual side only, both; taken or declined as the restatement says."""
    from dpft_amd.hip import ops
    o = L.sums_operands(c)
    M, K = c.M, c.K
    y, res, bnp, rbnp = _dev(o["y"]), _dev(o["res"]), _dev(o["bnp"]), _dev(o["rbnp"])
    ys = dict(y_sums=o["y_sums"].to(DEV), y_gamma=_dev(o["y_gamma"]), y_beta=_dev(o["y_beta"]))
    rs = dict(res_sums=o["res_sums"].to(DEV), res_gamma=_dev(o["res_gamma"]), res_beta=_dev(o["res_beta"]))
    want_form = L.sums_launch(M, K, sw)
    for side, kw in (("y", dict(ys, res_bnp=rbnp)), ("res", dict(rs, bnp=bnp)), ("both", dict(ys, **rs)), ("y-no-res", dict(ys))):
        what = "%s column sums on %s" % (c.name, side)
        has_res = side != "y-no-res"
        out, m8 = Guarded((M, K), torch.float32), Guarded((M, K // 4), torch.uint8)
        _, used = ops.bn_act_sums(y, res=res if has_res else None, eps=0.0, relu=True, out=out.t, mask8=m8.t, **kw)
        _form(ops, want_form, what)
        assert used == (want_form == "sums_taken"), what
        if used:
            want = L.ref_act(o["y"], o["bnp"], o["res"] if has_res else None, o["rbnp"] if has_res else None, True)
            _same(out.t, want, what + " out")
            _same(m8.t, L.mask_bytes(want), what + " mask8")
        else:
            assert out.untouched() and m8.untouched(), what + ": declined, but the outputs were written"
        assert out.intact() and m8.intact(), what + ": guard words overwritten"


def run_add_cvt():
    """add (both storage types, a tail of n % 4 elements in fp32) and the fp32 -> bf16 conversion: round to nearest even, ties
    and the largest finite values included."""
    from dpft_amd.hip import ops
    g = torch.Generator().manual_seed(5)
    for n in (4, 1028, 4096 * 4 + 4, 300 * 1024 + 12):
        src = torch.randn(n, generator=g) * 10.0 ** torch.randint(-6, 7, (n,), generator=g).float()
        src[:8] = torch.tensor([1.00390625, 1.01171875, -1.00390625, 3.3895313892515355e38, 0.0, -0.0, 2.0 ** -133, 1.0 + 2.0 ** -8 + 2.0 ** -20])[:min(8, n)]
        out = Guarded((n,), torch.bfloat16)
        ops.cvt_f32_bf16(_dev(src), out=out.t)
        _form(ops, "generic", "cvt n=%d" % n)
        _same(out.t, src.bfloat16().double(), "cvt n=%d" % n)
        assert out.intact()
        for dt, m in ((torch.float32, n + 3), (torch.bfloat16, n)):
            a64, b64 = torch.randint(-100, 100, (m,), generator=g).double(), torch.randint(-27, 28, (m,), generator=g).double() / 4
            a = Guarded((m,), dt)
            a.t.copy_(a64.to(dt))
            ops.add_any_(a.t, _dev(b64))
            want = (a64 + b64).float()
            _same(a.t, (want.bfloat16() if dt == torch.bfloat16 else want).double(), "add %s n=%d" % (dt, m))
            assert a.intact()


def run_float_case(c, sw, bf16):
    """Float tier: act and apply (sums from the reduce kernel itself) within c u T per element.  -> {what: worst error / bound}."""
    from dpft_amd.hip import ops
    o = L.float_operands(c)
    dt = torch.bfloat16 if bf16 else torch.float32
    y64, res64, dout64 = (L.to_storage(o[k], bf16) for k in ("y", "res", "dout"))
    y, res, dout, bnp, rbnp, gamma = _dev(y64, dt), _dev(res64, dt), _dev(dout64, dt), _dev(o["bnp"]), _dev(o["rbnp"]), _dev(o["gamma"])
    worst, fails = {}, []

    def check(got, want, terms, what):
        ratio = ((got.double().cpu() - want).abs() / L.float_bound(terms, want, bf16).clamp_min(1e-300))
        for i, name in enumerate(("r1", "r30", "r1000")):
            worst[what + ":" + name] = float(ratio[:, i::3].max())
            print("float tier %s %s %s %s: worst error / bound = %.3g" % (c.name, "bf16" if bf16 else "f32", what, name, worst[what + ":" + name]))
            if not worst[what + ":" + name] <= 1.0:
                fails.append((what, name, worst[what + ":" + name]))

    for v in L.ACT_VARIANTS:
        r, rb = (res64 if v["res"] else None), (o["rbnp"] if v["rbn"] else None)
        out = ops.bn_act_any(y, bnp, res if v["res"] else None, rbnp if v["rbn"] else None, v["relu"])
        _form(ops, L.elementwise_launch("act", c.M, c.K, bf16, sw).form, "%s float act" % c.name)
        check(out, L.ref_act(y64, o["bnp"], r, rb, v["relu"]), L.act_terms(y64, o["bnp"], r, rb),
              "act[%s]%s" % (ops.bn_last_form(), "".join(k for k in v if v[k])))
    m8 = torch.empty((c.M, c.K // 4), dtype=torch.uint8, device=DEV)
    ops.bn_act_any(y, bnp, res, None, True, mask8=m8)
    mask = L.mask_from_bytes(m8.cpu())
    sums = ops.bn_bwd_reduce_any(y, dout, bnp, mask8=m8)
    sums64 = sums.double().cpu()
    ref_sums = L.ref_reduce(y64, dout64, o["bnp"], mask)
    dz = torch.where(mask, dout64, torch.zeros_like(dout64))
    xhat = (y64 - o["bnp"][0]) * o["bnp"][3]
    # a sum of M terms in any order: (M + 2) u sum |terms| (2 roundings per term, M - 1 additions at most on any)
    sb = (c.M + 2) * L.U32 * torch.stack([dz.abs().sum(0), (dz * xhat).abs().sum(0)])
    worst["reduce"] = float(((sums64 - ref_sums).abs() / sb.clamp_min(1e-300)).max())
    if not worst["reduce"] <= 1.0:
        fails.append(("reduce", "", worst["reduce"]))
    for frozen in (False, True):
        dy = ops.bn_bwd_apply_any(y, dout, bnp, gamma, sums, mask8=m8, frozen=frozen)
        _form(ops, L.elementwise_launch("apply", c.M, c.K, bf16, sw).form, "%s float apply" % c.name)
        check(dy, L.ref_apply(y64, dout64, o["bnp"], o["gamma"], sums64, mask, frozen),
              L.apply_terms(y64, dout64, o["bnp"], o["gamma"], sums64, mask, frozen),
              "apply[%s]%s" % (ops.bn_last_form(), " frozen" if frozen else ""))
    return worst, fails


def run_all(sw, log=print):
    """Every case under the switches the process was started with (tools/bn_lattice_child.py)."""
    for c in L.LATTICE:
        run_case(c, sw)
    for c in L.POOL_LATTICE:
        run_pool_case(c, sw)
    for c in L.SUMS_CASES:
        run_sums_case(c, sw)
    run_add_cvt()
    torch.cuda.synchronize()
    log("bn lattice: %d + %d + %d cases under %s" % (len(L.LATTICE), len(L.POOL_LATTICE), len(L.SUMS_CASES), sw))
