"""The convolution kernels off the model's shapes: every case of the geometry lattice (tests/conv_lattice.py) through
dpft_amd.hip.ops, compared with torch.equal against the fp64 reference cast to fp32.

Integer operands make every summation order exact (see the lattice's docstring), so the fp32 MFMA kernels, the 3 x bf16 split
kernels and the bf16-operand kernels all have to return the same bits as fp64; one wrong border tap, one swapped row / column, one
unwritten pixel (outputs start as NaN) fails.  The kernel family the library reports for each launch is asserted too, so that a
case cannot pass on another kernel than the one it is here for.  One pass with randn operands under the project's float rule
(close() of tests/test_gpu_kernels.py) catches what integers cannot, e.g. an operand converted through the wrong type."""
import contextlib
import ctypes as C
import re

import pytest
import torch

from dpft_amd.hip.lib import HipLibraryError
from tests import conv_lattice as L

pytestmark = pytest.mark.gpu
DEV = "cuda"

MODES, FORCE_TILES, FORCE_WGRADS = L.MODES, L.FORCE_TILES, L.FORCE_WGRADS      # (shared with the host test of the launch plan)
CASES, C64, WVEC = list(L.LATTICE), L.C64, L.WVEC
_ids = lambda cs: [c.name for c in cs]


def close(a, b, rtol=1e-4, atol_scale=1e-5, what=""):      # the rule of tests/test_gpu_kernels.py, restated
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    atol = atol_scale * max(float(b.abs().max()), 1e-6)
    torch.testing.assert_close(a, b, rtol=rtol, atol=atol, msg=lambda m: f"{what}: {m}")


@contextlib.contextmanager
def compute_mode(name):
    from dpft_amd.hip import ops
    compute, split = MODES[name]
    try:
        ops.conv_set_compute(compute)
        ops.conv_set_split(split)
        yield ops
    finally:
        ops.conv_set_compute("fp32")
        ops.conv_set_split(True)
        ops._conv_cache.clear()


_data = {}


def case_data(c, float_pass=False):
    """Operands on the device and the fp64 references (kept in fp64 for the float pass, cast to fp32 on the device otherwise)."""
    key = (c.name, float_pass)
    if key not in _data:
        o = L.operands(c, float_pass)
        ref = L.reference(c, o)
        ref["y+bias"] = ref["y"] + o["bias"].double()
        ref["bnact"] = L.bnact_reference(ref["y"], o)
        ref["acc"] = ref["dx"] + o["base"].double()
        if c.C % 64 == 0:
            rp = L.reference(c, o, pro=True)
            ref["y_pro"], ref["dw_pro"] = rp["y"], rp["dw"]
        dev = {k: v.to(DEV) for k, v in o.items()}
        if not float_pass:
            for k, v in ref.items():
                assert float(v.abs().max()) < 2 ** 24 and torch.equal(v.float().double(), v), (c.name, k)
            ref = {k: v.float().to(DEV) for k, v in ref.items()}
        dev["unreached"] = L.unreached_mask(c).to(DEV)
        _data[key] = (dev, ref)
        if c.name in L.LARGE_NAMES and len(_data) > 8:      # keep the device footprint small
            for k in [k for k in _data if k != key][:4]:
                del _data[k]
    return _data[key]


def nan_like(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def run_case(ops, c, mode, tile=None, wtile=None, float_pass=False, parts=("fwd", "dgrad", "wgrad")):
    """Every form of the three operators on one case; returns nothing, asserts bit equality (or close() in the float pass)
    and the reported kernel family of every launch."""
    d, ref = case_data(c, float_pass)
    cv = ops.conv_problem(c.B, c.H, c.W, c.C, c.K, c.kh, c.kw, c.stride, c.pad)
    oh, ow = L.out_size(c)
    assert (cv.OH, cv.OW) == (oh, ow)
    got, want_fam = [], []

    def check(name, a, key, **tol):
        got.append((name, a, key, tol))

    ops.profile_start()
    if "fwd" in parts:
        fam = L.expected_family(c, "fwd", mode, tile)
        y, _ = ops.conv_fwd(cv, d["x"], d["w"], out=nan_like((c.B, oh, ow, c.K)))
        check("fwd", y, "y")
        y, _ = ops.conv_fwd(cv, d["x"], d["w"], bias=d["bias"], out=nan_like((c.B, oh, ow, c.K)))
        check("fwd + bias", y, "y+bias")
        want_fam += [("fwd", fam)] * 2
        if c.C % 64 == 0:
            y, _ = ops.conv_fwd(cv, d["x"], d["w"], pro=(d["pro"], True), want_stats=True, out=nan_like((c.B, oh, ow, c.K)))
            check("fwd + BatchNorm/ReLU prologue", y, "y_pro")
            want_fam.append(("fwd", fam))
        if L.refusal(c, L.BNACT):      # asserted refused (and nothing launched: no profile record)
            with pytest.raises(HipLibraryError, match=re.escape(L.refusal(c, L.BNACT))):
                ops.conv_fwd_bnact(cv, d["x"], d["w"], d["obn"], relu=True, residual=d["res"])
        else:
            from dpft_amd.hip.lib import lib, ptr, stream
            yb = nan_like((c.B, oh, ow, c.K))      # (ops.conv_fwd_bnact allocates its own output: the entry itself, as ops calls it)
            lib.call(L.BNACT, C.byref(cv.desc), ptr(d["x"]), ptr(d["w"]), ptr(d["obn"]), 1, ptr(d["res"]), ptr(yb),
                     ptr(ops.workspace(cv.ws_bytes, d["x"].device)), stream())
            check("fwd_bnact (+ residual, ReLU)", yb, "bnact")
            want_fam.append(("fwd", fam))
    if "dgrad" in parts:
        fam = L.expected_family(c, "dgrad", mode, tile)
        wt = ops.weight_transpose(d["w"])
        dx = ops.conv_dgrad(cv, d["dy"], wt, out=nan_like((c.B, c.H, c.W, c.C)), accumulate=False)
        check("dgrad", dx, "dx")
        acc = ops.conv_dgrad(cv, d["dy"], wt, out=d["base"].clone(), accumulate=True)
        check("dgrad accumulate", acc, "acc", rtol=1e-3, atol_scale=1e-4)
        want_fam += [("dgrad", fam)] * 2
        if c.stride > 1 and c.K % 64 == 0 and c.C > 4:
            # without a workspace a strided data gradient cannot split K: one launch per parity class, whatever the map size
            from dpft_amd.hip.lib import lib, ptr, stream
            dx0 = nan_like((c.B, c.H, c.W, c.C))
            lib.call("dpft_conv2d_nhwc_dgrad_f32", C.byref(cv.desc), ptr(d["dy"]), ptr(wt), ptr(dx0), 0, None, stream())
            check("dgrad, parity classes", dx0, "dx")
            acc0 = d["base"].clone()
            lib.call("dpft_conv2d_nhwc_dgrad_f32", C.byref(cv.desc), ptr(d["dy"]), ptr(wt), ptr(acc0), 1, None, stream())
            check("dgrad accumulate, parity classes", acc0, "acc", rtol=1e-3, atol_scale=1e-4)
            want_fam += [("dgrad", L.expected_family(c, "dgrad", mode, tile, workspace=False))] * 2
    if "wgrad" in parts:
        fam = L.expected_family(c, "wgrad", mode, wtile=wtile)
        check("wgrad", ops.conv_wgrad(cv, d["x"], d["dy"], out=nan_like((c.K, c.kh, c.kw, c.C))), "dw")
        want_fam.append(("wgrad", fam))
        if c.C % 64 == 0 and L.refusal(c, L.WGRAD_PRO):      # asserted refused (nothing launched: no profile record)
            with pytest.raises(HipLibraryError, match=re.escape(L.refusal(c, L.WGRAD_PRO))):
                ops.conv_wgrad(cv, d["x"], d["dy"], pro=(d["pro"], True))
        elif c.C % 64 == 0:
            dw = ops.conv_wgrad(cv, d["x"], d["dy"], pro=(d["pro"], True), out=nan_like((c.K, c.kh, c.kw, c.C)))
            check("wgrad + prologue", dw, "dw_pro")
            want_fam.append(("wgrad", fam))
        if c.K <= 256:
            dw, db = ops.conv_wgrad_bias(cv, d["x"], d["dy"], out=nan_like((c.K, c.kh, c.kw, c.C)), bias_out=nan_like((c.K,)))
            check("wgrad_bias: dw", dw, "dw")
            check("wgrad_bias: db", db, "db")
            want_fam.append(("wgrad", fam))
    recs = ops.profile_collect()
    bad = []
    for name, a, key, tol in got:
        if float_pass:
            close(a, ref[key], what=f"{c.name} [{mode}] {name}", **tol)
        elif not torch.equal(a, ref[key]):
            diff = (a.double() - ref[key].double())
            n_bad = int((diff != 0).sum() + diff.isnan().sum())
            bad.append(f"{name}: {n_bad} of {a.numel()} entries differ (max |diff| {float(diff.nan_to_num(1e30).abs().max()):g})")
        if key in ("dx",) and not float_pass:
            z = a[:, d["unreached"]]
            if z.numel() and not bool((z == 0).all()):
                bad.append(f"{name}: input pixels no tap reaches are not 0.0")
    assert not bad, (tuple(c), mode, tile, wtile, bad)
    fams = [(r[0], r[4]) for r in recs]
    assert fams == want_fam, (tuple(c), mode, tile, wtile, fams, want_fam)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_lattice_case_equals_fp64_bit_for_bit(case, mode):
    with compute_mode(mode) as ops:
        run_case(ops, case, mode)


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("tile", FORCE_TILES)
@pytest.mark.parametrize("case", C64, ids=_ids(C64))
def test_forced_tiles_forward_and_data_gradient(case, tile, mode, monkeypatch):
    """Every tile shape and a K split on the small, ragged geometries; in bf16x3 mode a forced tile sends the problem to the
    split kernels of conv_x3.hip."""
    monkeypatch.setenv("DPFT_FORCE_TILE", tile)
    with compute_mode(mode) as ops:
        ops._conv_cache.clear()
        run_case(ops, case, mode, tile=tuple(int(v) for v in tile.split(",")), parts=("fwd", "dgrad"))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("wtile", FORCE_WGRADS)
@pytest.mark.parametrize("case", WVEC, ids=_ids(WVEC))
def test_forced_weight_gradient_tiles(case, wtile, mode, monkeypatch):
    monkeypatch.setenv("DPFT_FORCE_WGRAD", wtile)
    with compute_mode(mode) as ops:
        ops._conv_cache.clear()
        run_case(ops, case, mode, wtile=tuple(int(v) for v in wtile.split(",")), parts=("wgrad",))


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_lattice_case_float_pass(case):
    """randn operands, default mode, the project's element-by-element rule."""
    with compute_mode("fp32+split") as ops:
        run_case(ops, case, "fp32+split", float_pass=True)


GUARD = 65536
_WS_CONFIGS = [("default", None, None)] + [("tile " + t, t, None) for t in FORCE_TILES] + [("wgrad " + t, None, t) for t in FORCE_WGRADS]


@pytest.mark.parametrize("cfg", _WS_CONFIGS, ids=[c[0].replace(" ", "=") for c in _WS_CONFIGS])
@pytest.mark.parametrize("mode", ["fp32", "fp32+split", "bf16x3"])
def test_workspace_contract_exact_size_guard_and_ticket_header(cfg, mode, monkeypatch):
    """ops.workspace hands out 1.25 x the size the library asks for; here every entry point gets EXACTLY
    dpft_conv2d_workspace_bytes bytes, followed inside the same allocation by a 64 KiB guard: the guard is unchanged
    afterwards, the ticket header is all zero again, and the results are still the fp64 bits (the slabs start as NaN)."""
    from dpft_amd.hip.lib import lib, make_desc, ptr, stream
    _, tile, wtile = cfg
    if tile:
        monkeypatch.setenv("DPFT_FORCE_TILE", tile)
    if wtile:
        monkeypatch.setenv("DPFT_FORCE_WGRAD", wtile)
    cases = CASES if not (tile or wtile) else (C64 if tile else WVEC)
    hdr = int(lib.dpft_conv2d_workspace_header_bytes())
    assert hdr > 0
    bad = []
    with compute_mode(mode) as ops:
        for c in cases:
            d, ref = case_data(c)
            desc = make_desc(c.B, c.H, c.W, c.C, c.K, c.kh, c.kw, c.stride, c.pad)
            nbytes = int(lib.dpft_conv2d_workspace_bytes(C.byref(desc)))
            assert nbytes >= hdr, (c, nbytes)
            buf = torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)      # slabs: NaN patterns
            buf[nbytes:] = 0xA5
            ws = C.c_void_p(buf.data_ptr())
            lib.call("dpft_conv2d_workspace_init", ws, stream())
            oh, ow = L.out_size(c)
            y = nan_like((c.B, oh, ow, c.K))
            out = {}
            lib.call("dpft_conv2d_nhwc_fwd_f32", C.byref(desc), ptr(d["x"]), ptr(d["w"]), ptr(d["bias"]), None, 0, ptr(y), None, ws, stream())
            out["y+bias"] = y
            if c.C % 64 == 0:
                tiles = int(lib.dpft_conv2d_stats_tiles(C.byref(desc), None))
                stats = nan_like((tiles, 2, c.K))
                y2 = nan_like((c.B, oh, ow, c.K))
                lib.call("dpft_conv2d_nhwc_fwd_f32", C.byref(desc), ptr(d["x"]), ptr(d["w"]), None, ptr(d["pro"]), 1, ptr(y2), ptr(stats), ws, stream())
                out["y_pro"] = y2
            if not L.refusal(c, L.BNACT):
                y3 = nan_like((c.B, oh, ow, c.K))
                lib.call("dpft_conv2d_nhwc_fwd_bnact_f32", C.byref(desc), ptr(d["x"]), ptr(d["w"]), ptr(d["obn"]), 1, ptr(d["res"]), ptr(y3), ws, stream())
                out["bnact"] = y3
            wt = ops.weight_transpose(d["w"])
            dx = nan_like((c.B, c.H, c.W, c.C))
            lib.call("dpft_conv2d_nhwc_dgrad_f32", C.byref(desc), ptr(d["dy"]), ptr(wt), ptr(dx), 0, ws, stream())
            out["dx"] = dx
            acc = d["base"].clone()
            lib.call("dpft_conv2d_nhwc_dgrad_f32", C.byref(desc), ptr(d["dy"]), ptr(wt), ptr(acc), 1, ws, stream())
            out["acc"] = acc
            dw = nan_like((c.K, c.kh, c.kw, c.C))
            lib.call("dpft_conv2d_nhwc_wgrad_f32", C.byref(desc), ptr(d["x"]), ptr(d["dy"]), None, 0, ptr(dw), ws, stream())
            out["dw"] = dw
            if c.K <= 256:
                dw2, db = nan_like((c.K, c.kh, c.kw, c.C)), nan_like((c.K,))
                lib.call("dpft_conv2d_nhwc_wgrad_bias_f32", C.byref(desc), ptr(d["x"]), ptr(d["dy"]), ptr(dw2), ptr(db), ws, stream())
                out["db"], out["dw_bias"] = db, dw2
            if c.C % 64 == 0 and not L.refusal(c, L.WGRAD_PRO):
                dw3 = nan_like((c.K, c.kh, c.kw, c.C))
                lib.call("dpft_conv2d_nhwc_wgrad_f32", C.byref(desc), ptr(d["x"]), ptr(d["dy"]), ptr(d["pro"]), 1, ptr(dw3), ws, stream())
                out["dw_pro"] = dw3
            torch.cuda.synchronize()
            if not bool((buf[nbytes:] == 0xA5).all()):
                bad.append((c.name, "guard overwritten", nbytes))
            if int(buf[:hdr].count_nonzero()) != 0:
                bad.append((c.name, "ticket header not zero"))
            for k, v in out.items():
                if not torch.equal(v, ref["dw" if k == "dw_bias" else k]):
                    bad.append((c.name, k, "differs from fp64"))
    assert not bad, (cfg[0], mode, bad)
