"""GPU half of tests/stats_lattice.py: one forward conv launch at a time through the C entries, its per-tile statistics table (and
the fixed-point column sums) against the fp64 reference, bounds and plan restatement of that file.  Used in process by
tests/test_gpu_conv_stats.py and tests/test_gpu_bn_stats.py and, with DPFT_SK_FIXUP=0, by tools/conv_stats_child.py.  Every
function raises AssertionError with the case and the launch in its message; WORST collects the worst error / bound per form."""
import ctypes as C
import os
import re

import numpy as np
import torch

from tests import conv_lattice as L
from tests import stats_lattice as S
from tests.bn_passes_driver import Guarded

DEV = "cuda"
FAMILY = {"stream": "f32", "generic": "vector", "pipe": "f32", "x3": "x3", "vec": "bf16"}
WORST = {}      # form -> [worst mean ratio, worst M2 ratio] (sums: units beyond the restated value / slack)
EPS = 1e-5


def note(form, *ratios):
    w = WORST.setdefault(form, [0.0] * len(ratios))
    for i, r in enumerate(ratios):
        w[i] = max(w[i], float(r))


def report():
    return "; ".join("%s %s" % (k, "/".join("%.3f" % v for v in w)) for k, w in sorted(WORST.items()))


class mode_ctx:
    """Compute mode and split switch of a launch group (and DPFT_FORCE_TILE where the caller has not set it through monkeypatch)."""

    def __init__(self, mode, tile=None, set_env=False):
        self.mode, self.tile, self.set_env = mode, tile, set_env

    def __enter__(self):
        from dpft_amd.hip import ops
        if self.set_env and self.tile:
            os.environ["DPFT_FORCE_TILE"] = self.tile
        assert os.environ.get("DPFT_FORCE_TILE") == self.tile, (os.environ.get("DPFT_FORCE_TILE"), self.tile)
        compute, split = L.MODES[self.mode]
        ops.conv_set_compute(compute)
        ops.conv_set_split(split)
        ops._conv_cache.clear()
        return ops

    def __exit__(self, *exc):
        from dpft_amd.hip import ops
        if self.set_env:
            os.environ.pop("DPFT_FORCE_TILE", None)
        ops.conv_set_compute("fp32")
        ops.conv_set_split(True)
        ops._conv_cache.clear()


_dev = {}


def device_case(c):
    """Operands and both exact outputs (without / with the prologue) of a case on the device."""
    if c.name not in _dev:
        if len(_dev) > 24:
            _dev.clear()
        o = L.operands(c)
        d = {k: o[k].to(DEV) for k in ("x", "w", "bias", "pro")}
        for pro in ((False, True) if c.C % 64 == 0 else (False,)):
            y = S.case_output(c, pro)[0]
            assert float(np.abs(y).max()) < 2 ** 24
            d["y", pro] = torch.from_numpy(y).float().view(c.B, *L.out_size(c), c.K).to(DEV)
        _dev[c.name] = d
    return _dev[c.name]


def nan_like(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _tag(l, what=""):
    return "%s [%s, tile %s, %s] %s" % (l.case.name, l.mode, l.tile, "prologue" if l.pro else "no prologue", what)


def _problem(ops, c):
    return ops.conv_problem(c.B, c.H, c.W, c.C, c.K, c.kh, c.kw, c.stride, c.pad)


def _fwd(ops, cv, d, l, y, stats, bias=None):
    from dpft_amd.hip.lib import lib, ptr, stream
    lib.call("dpft_conv2d_nhwc_fwd_f32", C.byref(cv.desc), ptr(d["x"]), ptr(d["w"]), ptr(bias), ptr(d["pro"]) if l.pro else None,
             int(l.pro), ptr(y), ptr(stats), ptr(ops.workspace(cv.ws_bytes, d["x"].device)), stream())


def _fwd_sums(ops, cv, d, l, y, stats, acc, bias=None, pro_bn=None, pro_sums=None):
    """-> (sums used, prologue sums used); pro_sums = (words (4, C) int64, gamma, beta, rows)."""
    from dpft_amd.hip.lib import lib, ptr, stream
    used, pused = C.c_int32(-1), C.c_int32(-1)
    pb = pro_bn if pro_bn is not None else (d["pro"] if l.pro else None)
    ps = pro_sums or (None, None, None, 1)
    lib.call("dpft_conv2d_nhwc_fwd_sums_f32", C.byref(cv.desc), ptr(d["x"]), ptr(d["w"]), ptr(bias), ptr(pb), int(pb is not None),
             ptr(y), ptr(stats), ptr(acc), C.byref(used), ptr(ps[0]), ptr(ps[1]), ptr(ps[2]), int(ps[3]), EPS, C.byref(pused),
             ptr(ops.workspace(cv.ws_bytes, d["x"].device)), stream())
    return used.value, pused.value


class Words:
    """(4, K) zeroed 64-bit accumulator words between guard words."""
    GUARD, SENTINEL = 64, 0x5A5A5A5A5A5A

    def __init__(self, K):
        self.buf = torch.full((4 * K + 2 * self.GUARD,), self.SENTINEL, dtype=torch.int64, device=DEV)
        self.t = self.buf[self.GUARD:self.GUARD + 4 * K].view(4, K)
        self.t.zero_()

    def intact(self):
        return bool((torch.cat([self.buf[:self.GUARD], self.buf[-self.GUARD:]]) == self.SENTINEL).all())


def run_launch(ops, l, child=False):
    """The per-launch assertions of the table; -> (fp32 table as numpy, y of the launch without statistics)."""
    from dpft_amd.hip.lib import lib
    c = l.case
    p, ref = S.launch_reference(l, child)
    d = device_case(c)
    cv = _problem(ops, c)
    tr = C.c_int32(0)
    tiles = int(lib.dpft_conv2d_stats_tiles(C.byref(cv.desc), C.byref(tr)))
    assert (tr.value, tiles) == (p.bm, -(-L.rows(c) // p.bm)), _tag(l, "tile rows %d x %d tiles, the plan says %d rows" % (tr.value, tiles, p.bm))
    shape = (c.B, *L.out_size(c), c.K)
    ops.profile_start()
    y0 = nan_like(shape)
    _fwd(ops, cv, d, l, y0, None)
    tab = Guarded((tiles, 2, c.K), torch.float32)
    y1 = nan_like(shape)
    _fwd(ops, cv, d, l, y1, tab.t)
    fams = [(r[0], r[4]) for r in ops.profile_collect()]
    assert fams == [("fwd", FAMILY[p.kernel])] * 2, _tag(l, "ran as %s, the plan says %s (%s)" % (fams, FAMILY[p.kernel], S.form_name(p)))
    assert torch.equal(y0, d["y", l.pro]), _tag(l, "y differs from fp64")
    assert torch.equal(y1, y0), _tag(l, "y with statistics differs from y without")
    assert tab.intact(), _tag(l, "guard around the table overwritten")
    table = tab.t.cpu().numpy()
    bad, ratios = S.check_table(table, ref)
    assert not bad, _tag(l, "%s: %s" % (S.form_name(p), bad))
    note(S.form_name(p), *ratios)
    return table, y0


def run_sums(ops, l, table, y0, child=False):
    """The same launch through dpft_conv2d_nhwc_fwd_sums_f32: taken or declined as the plan says; the accumulator words."""
    c = l.case
    p = S.launch_plan(l, sums=True, child=child)
    counts = S.tile_counts(L.rows(c), p.bm)
    d = device_case(c)
    cv = _problem(ops, c)
    shape = (c.B, *L.out_size(c), c.K)

    def launch(acc, bias=None):
        tab, y = Guarded(table.shape, torch.float32), nan_like(shape)
        used, _ = _fwd_sums(ops, cv, d, l, y, tab.t, acc.t, bias=bias)
        assert tab.intact() and acc.intact(), _tag(l, "sums: guard overwritten")
        return used, tab, y
    acc = Words(c.K)
    used, tab, y = launch(acc)
    assert used == int(p.stat_sums), _tag(l, "sums used = %d, the plan (%s) says %d" % (used, S.form_name(p), p.stat_sums))
    assert torch.equal(y, y0), _tag(l, "sums: y differs")
    if not used:
        assert int(acc.t.count_nonzero()) == 0, _tag(l, "sums declined, accumulator written")
        assert np.array_equal(tab.t.cpu().numpy().view(np.int32), table.view(np.int32)), _tag(l, "sums declined: the table differs")
    else:
        words = acc.t.cpu().numpy().copy()
        u1, u2 = S.decode_units(words)
        e1, e2, slack = S.sums_expected(table, counts)
        off1 = [int(a) - int(b) for a, b in zip(u1, e1)]
        assert not any(off1), _tag(l, "sum 1 differs from the encoded sum of cnt * mean: first %r" % next((i, v) for i, v in enumerate(off1) if v))
        off2 = [abs(int(a) - int(b)) / s for a, b, s in zip(u2, e2, slack)]
        assert max(off2) <= 1.0, _tag(l, "sum 2: %.3f of the bound at channel %d" % (max(off2), int(np.argmax(off2))))
        note("sums " + S.form_name(p), max(off2))
        used2, _, _ = launch(acc)      # a second launch into the same words: the integer sum
        assert used2 == 1 and np.array_equal(acc.t.cpu().numpy(), words + words), _tag(l, "two launches into one accumulator are not twice one")
        again = Words(c.K)
        launch(again)
        assert np.array_equal(again.t.cpu().numpy(), words), _tag(l, "two runs of one launch give different words")
    if p.kernel != "stream":      # with a bias: declined by every kernel (the streaming kernel takes no bias with statistics at all)
        acc = Words(c.K)
        used, tab, y = launch(acc, bias=d["bias"])
        assert used == 0 and int(acc.t.count_nonzero()) == 0, _tag(l, "sums with a bias: used %d" % used)
        assert bool(torch.isfinite(tab.t).all()), _tag(l, "sums with a bias: the table is not written")
        assert torch.equal(y, y0 + d["bias"]), _tag(l, "sums with a bias: y differs")


def producer_sums(c):
    """Column sums of the conv's INPUT x (as the producing layer's accumulators would hold them: integers, nothing truncated)
    with gamma / beta of the lattice's prologue block -> (words (4, C) on the device, gamma, beta, rows)."""
    o = S.case_output(c, True)[2]
    x = o["x"].double().reshape(-1, c.C).numpy()
    words = torch.from_numpy(S.encode_words(x.sum(0), (x * x).sum(0))).to(DEV)
    return words, o["pro"][1].contiguous().to(DEV), o["pro"][2].contiguous().to(DEV), x.shape[0]


def finalize_sums(layers, momentum=0.1, running=True):
    """dpft_bn_finalize_sums_f32 over ``layers`` = [(words (4, K) device int64, gamma, beta, M, rm, rv)]; -> (rc, [bnp])."""
    from dpft_amd.hip.lib import lib, stream
    n = len(layers)
    arr = lambda ts: (C.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])
    outs = [Guarded((4, w.shape[1]), torch.float32) for w, *_ in layers]
    Ms = (C.c_int64 * n)(*[l[3] for l in layers])
    Ks = (C.c_int32 * n)(*[l[0].shape[1] for l in layers])
    rc = lib.dpft_bn_finalize_sums_f32(n, arr([l[0] for l in layers]), arr([l[1] for l in layers]), arr([l[2] for l in layers]),
                                       arr([l[4] if running else None for l in layers]), arr([l[5] if running else None for l in layers]),
                                       arr([o.t for o in outs]), Ms, Ks, EPS, momentum, stream())
    torch.cuda.synchronize()
    return rc, outs


def run_pro_from_sums(ops, l):
    """A conv whose prologue comes as column sums against the same conv given the BN block dpft_bn_finalize_sums_f32 makes of
    those sums: bit-identical where the plan offers it, refused elsewhere (nothing written)."""
    from dpft_amd.hip.lib import HipLibraryError
    assert l.pro
    c = l.case
    p = S.launch_plan(l)
    d = device_case(c)
    cv = _problem(ops, c)
    words, gamma, beta, rows = producer_sums(c)
    rc, (blk,) = finalize_sums([(words, gamma, beta, rows, None, None)], running=False)
    assert rc == 0 and blk.intact() and bool(torch.isfinite(blk.t).all()), _tag(l, "finalize of the producer's sums")
    shape = (c.B, *L.out_size(c), c.K)
    ya = nan_like(shape)
    if not p.pro_from_sums:
        with_err = None
        try:
            _fwd_sums(ops, cv, d, l, ya, None, None, pro_bn=blk.t, pro_sums=(words, gamma, beta, rows))
        except HipLibraryError as e:
            with_err = str(e)
        assert with_err and "builds no prologue from column sums" in with_err, _tag(l, "prologue from sums not refused: %r" % with_err)
        assert bool(torch.isnan(ya).all()), _tag(l, "refused, but y is written")
        return False
    _, pused = _fwd_sums(ops, cv, d, l, ya, None, None, pro_bn=blk.t, pro_sums=(words, gamma, beta, rows))
    assert pused == 1, _tag(l, "prologue sums used = %d" % pused)
    yb = nan_like(shape)
    _fwd_sums(ops, cv, d, l, yb, None, None, pro_bn=blk.t)
    assert bool(torch.isfinite(yb).all()) and torch.equal(ya, yb), _tag(l, "prologue from sums differs from the prologue from the finalized block (%s)" % S.form_name(p))
    # and the block is the BatchNorm of x: the conv is not the one without a prologue (unless no tap reaches anything: y = 0)
    assert not torch.equal(yb, d["y", False]) or not bool(yb.any()), _tag(l, "the prologue changed nothing")
    return True


def run_stream_refusal(ops, c, mode):
    """Statistics with a bias on a streaming shape: DPFT_ERR_ARG and nothing written."""
    from dpft_amd.hip.lib import HipLibraryError
    l = S.Launch(c, mode, None, False)
    d = device_case(c)
    cv = _problem(ops, c)
    y, tab = nan_like((c.B, *L.out_size(c), c.K)), Guarded((cv.tiles, 2, c.K), torch.float32)
    err = None
    try:
        _fwd(ops, cv, d, l, y, tab.t, bias=d["bias"])
    except HipLibraryError as e:
        err = str(e)
    assert err and re.search("statistics of a streaming 1x1 conv", err), _tag(l, "not refused: %r" % err)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and tab.untouched() and tab.intact(), _tag(l, "refused, but something is written")


def run_group(mode, tile, child=False, set_env=False, sums=False, launches=None):
    with mode_ctx(mode, tile, set_env) as ops:
        for l in (launches if launches is not None else S.group_launches(mode, tile)):
            table, y0 = run_launch(ops, l, child)
            if sums:
                run_sums(ops, l, table, y0, child)


# ---------------------------------------------------------------------------------------------------------------------------------
# bn_stats_kernel / bn_finalize_kernel directly
# ---------------------------------------------------------------------------------------------------------------------------------
def _within(got, ref_bound, what, form):
    ref, bound = ref_bound
    err = np.abs(got.double().cpu().numpy() - ref)
    ok = err <= bound
    assert bool(ok.all()), "%s: %d entries beyond the bound, first %r: |d| %.3e > %.3e" % (
        what, int((~ok).sum()), tuple(np.argwhere(~ok)[0]), err[~ok][0], bound[~ok][0])
    pos = bound > 0
    note(form, float((err[pos] / bound[pos]).max()) if pos.any() else 0.0)


def _params(K, seed):
    g = torch.Generator().manual_seed(seed)
    gamma, beta = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g)
    rm, rv = torch.randn(K, generator=g), torch.rand(K, generator=g) + 0.5
    return [t.to(DEV) for t in (gamma, beta, rm, rv)]


def run_bn_exact(case):
    from dpft_amd.hip import ops
    M, K, tr = case
    y = S.exact_data(M, K, tr)
    table = S.tile_table(y, tr)
    counts = S.tile_counts(M, tr)
    stats = ops.bn_stats(torch.from_numpy(y).float().to(DEV), tr)
    what = "bn exact tier M=%d K=%d tile_rows=%d" % case
    assert tuple(stats.shape) == table.shape and np.array_equal(stats.cpu().numpy(), table.astype(np.float32)), what + ": the table differs from fp64"
    gamma, beta, rm, rv = _params(K, 11 + M + K)
    bnp = ops.bn_finalize(stats, tr, M, gamma, beta, EPS, 1.0, rm, rv)
    mean, m2 = S.merge_table(table, counts)
    var = m2 / M
    assert np.array_equal(bnp[0].cpu().numpy(), mean.astype(np.float32)), what + ": mean"
    assert torch.equal(bnp[2], beta), what + ": beta"
    assert np.array_equal(rm.cpu().numpy(), mean.astype(np.float32)), what + ": running_mean at momentum 1 is not the mean"
    unb = (m2.astype(np.float32) / np.float32(M - 1)) if M > 1 else var.astype(np.float32)      # M2 is an fp32 value: one division
    assert np.array_equal(rv.cpu().numpy(), unb), what + ": running_var at momentum 1 is not the correctly rounded M2 / (M - 1)"
    # invstd = 1 / sqrtf(var + eps) of an exact var: the sum, the root (half weight) and the reciprocal round
    invstd = 1.0 / np.sqrt(var + EPS)
    e_inv = invstd * 3 * S.U
    _within(bnp[3], (invstd, e_inv), what + ": invstd", "finalize exact invstd")
    g64 = gamma.double().cpu().numpy()
    _within(bnp[1], (g64 * invstd, np.abs(g64) * e_inv + S.U * np.abs(g64 * invstd)), what + ": scale", "finalize exact scale")


def run_bn_float(case):
    from dpft_amd.hip import ops
    M, K, tr = case
    y = S.float_data(M, K)
    what = "bn float tier M=%d K=%d tile_rows=%d" % case
    stats = ops.bn_stats(torch.from_numpy(y).to(DEV), tr)
    table, e_m, e_m2 = S.bn_stats_bounds(y, tr)
    assert tuple(stats.shape) == table.shape and bool(torch.isfinite(stats).all()), what
    _within(stats[:, 0], (table[:, 0], e_m), what + ": tile mean", "bn_stats mean")
    _within(stats[:, 1], (table[:, 1], e_m2), what + ": tile M2", "bn_stats M2")
    gamma, beta, rm, rv = _params(K, 13 + M + K)
    rm0, rv0 = rm.double().cpu().numpy(), rv.double().cpu().numpy()
    bnp = ops.bn_finalize(stats, tr, M, gamma, beta, EPS, 0.1, rm, rv)
    b = S.finalize_bounds(stats.cpu().numpy(), S.tile_counts(M, tr), M, gamma.double().cpu().numpy(), EPS, 0.1, rm0, rv0)
    _within(bnp[0], b["mean"], what + ": mean", "finalize mean")
    _within(bnp[3], b["invstd"], what + ": invstd", "finalize invstd")
    _within(bnp[1], b["scale"], what + ": scale", "finalize scale")
    assert torch.equal(bnp[2], beta), what + ": beta"
    _within(rm, b["rm"], what + ": running_mean", "finalize running_mean")
    _within(rv, b["rv"], what + ": running_var", "finalize running_var")
    # end to end against the data: the table's own error on top (mean: the tile means' bound; variance: M2's, relative)
    mean64, var64 = S.merged(y.astype(np.float64))
    e2e = b["mean"][1] + e_m.max(0)
    assert bool((np.abs(bnp[0].double().cpu().numpy() - mean64) <= e2e).all()), what + ": mean against the data"
    if M > 1:
        rel = np.abs(bnp[3].double().cpu().numpy() * np.sqrt(var64 + EPS) - 1.0)
        assert float(rel.max()) < 1e-4, what + ": invstd against the data: %.3e" % float(rel.max())


def run_finalize_sums():
    """Two layers of different K in one launch (the kmax grid, the c >= K guard), BN block and running statistics from the decoded
    sums in rational arithmetic; 48 layers accepted, 49 refused."""
    from dpft_amd.hip.lib import lib
    layers, refs = [], []
    for M, K in ((300, 96), (4209, 320), (1, 12)):
        y = S.float_data(M, K, seed=3).astype(np.float64)
        words = S.encode_words(y.sum(0), (y * y).sum(0))
        gamma, beta, rm, rv = _params(K, 17 + K)
        u1, u2 = S.decode_units(words)
        refs.append(S.sums_finalize_bounds(u1, u2, M, gamma.double().cpu().numpy(), beta.double().cpu().numpy(), EPS, 0.1,
                                           rm.double().cpu().numpy(), rv.double().cpu().numpy()))
        layers.append((torch.from_numpy(words).to(DEV), gamma, beta, M, rm, rv))
    rc, outs = finalize_sums(layers)
    assert rc == 0, lib.dpft_last_error()
    for (w, gamma, beta, M, rm, rv), out, b in zip(layers, outs, refs):
        what = "finalize sums M=%d K=%d" % (M, w.shape[1])
        assert out.intact() and bool(torch.isfinite(out.t).all()), what + ": guard / unwritten"
        _within(out.t[0], b["mean"], what + ": mean", "finalize sums mean")
        _within(out.t[3], b["invstd"], what + ": invstd", "finalize sums invstd")
        _within(out.t[1], b["scale"], what + ": scale", "finalize sums scale")
        assert torch.equal(out.t[2], beta), what + ": beta"
        _within(rm, b["rm"], what + ": running_mean", "finalize sums running_mean")
        _within(rv, b["rv"], what + ": running_var", "finalize sums running_var")
    small = layers[2][:4] + (None, None)
    rc, outs = finalize_sums([small] * 48, running=False)
    assert rc == 0 and all(torch.equal(o.t, outs[0].t) and o.intact() for o in outs), "48 layers"
    _within(outs[0].t[0], refs[2]["mean"], "48 layers: mean", "finalize sums mean")
    rc, outs = finalize_sums([small] * 49, running=False)
    assert rc == -1 and b"1..48 layers" in lib.dpft_last_error() and all(o.untouched() for o in outs), (rc, lib.dpft_last_error())


def run_child():
    """Everything that needs DPFT_SK_FIXUP=0 (read once per process): the forced K splits end in a reduction launch."""
    assert os.environ.get("DPFT_SK_FIXUP") == "0"
    for mode, tile in S.CHILD_GROUPS:
        run_group(mode, tile, child=True, set_env=True, sums=True)
    missing = set(S.REQUIRED_CHILD_FORMS) - set(WORST)
    assert not missing, missing
    print("worst error / bound per form:", report())
