"""The row-shared main loop of the split 3x3 kernels (dpft_amd/csrc/conv_x3r.hip: the A tile staged once per filter row, the three
taps of the row read at row offsets 0, 1, 2) against fp64, with the switch DPFT_X3_ROW3 on and off in one process.

What can go wrong there and nowhere else: the wrap from one image row into the next (masked on the fragments: W = 1, 2, 3, 5 wrap
many times inside a tile, 57 a few times), vertical borders and batch seams inside a tile (decided at staging: H = 1, 2, 3, B = 3
with H W < 128), the two halo rows of a stage (M below, equal to and not a multiple of the tile), the K split at (filter row, K-slice)
boundaries, the flipped taps of the data gradient, and the zero that padding keeps BEHIND BatchNorm + ReLU (beta > 0, some gamma < 0).
The kernels are reached through the C ABI the way tests/test_gpu_conv_x3.py reaches them: compute mode bf16x3 + DPFT_FORCE_TILE.

Gate: the two conditions of tests/test_gpu_conv_x3.py::test_split_mode_error_not_above_the_fp32_mfma_paths -- relative L2 error
against fp64 below ABS_BOUND = 2e-6 and not above the fp32 MFMA path's error times FACTOR = 1.02 (+ 1e-9) -- and that test's
statistics form (mean within 1e-5 of the largest |y|).  Accumulation order differs between the two forms, so bit equality is not
asked; the switch-off error is printed beside the new one.  (The operand prologue of a 3x3 / pad 1 conv is always the padded form,
PRO_ = 2; PRO_ = 1 belongs to the unpadded 1x1 convs, which stay on their kernels.)

Measured (MI355X), worst relative L2 error over all cases, row-shared / per-tap / fp32 MFMA: forward 1.74e-7 / 1.78e-7 / 3.05e-7, forward
+ prologue (also with column sums) 1.54e-7 / 1.54e-7 / 2.56e-7, data gradient (also with the BatchNorm-backward reduction) 1.77e-7 /
1.77e-7 / 4.27e-7, residual form 1.40e-7 / 1.40e-7; the row-shared error is at most 0.65 of the fp32 MFMA path's in any case."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
ABS_BOUND, FACTOR = 2e-6, 1.02      # test_split_mode_error_not_above_the_fp32_mfma_paths: `< 2e-6`, `lim = 1.02` (forward, data gradient)

# (B, H, W): M = 1 | 6 | 6 | 45 (seams inside a tile) | 342 (three 128-row tiles, ragged) | 128 = one tile, W = 2 | 171 | 129, W = 1
GEOMS = [(1, 1, 1), (3, 1, 2), (1, 2, 3), (3, 3, 5), (3, 2, 57), (2, 32, 2), (1, 3, 57), (3, 43, 1)]
# (GEMM reduction channels, GEMM columns, K split): the columns pick the tile -- 64: 64 x 64, 128: 128 x 64, 256: 128 x 128
CONFIGS = [(64, 64, 1), (64, 128, 2), (128, 256, 1), (128, 64, 2), (64, 256, 2), (128, 128, 1)]
TILE = {64: "64,64", 128: "128,64", 256: "128,128"}


def _rel(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).norm() / (ref.norm() + 1e-300))


def _mask8(bits):
    B, H, W, C_ = bits.shape
    return (bits.view(B, H, W, C_ // 4, 4).to(torch.uint8) * torch.tensor([1, 2, 4, 8], dtype=torch.uint8)).sum(-1).to(torch.uint8).contiguous()


def _mean_from_sums(acc, M, K):
    """dpft_bn_finalize_sums_f32 of one layer's column sums -> the mean row of its BN block."""
    from dpft_amd.hip.lib import lib, stream
    ones, zeros, bnp = torch.ones(K, device=DEV), torch.zeros(K, device=DEV), torch.empty(4, K, device=DEV)
    arr = lambda t: (C.c_void_p * 1)(None if t is None else t.data_ptr())
    rc = lib.dpft_bn_finalize_sums_f32(1, arr(acc), arr(ones), arr(zeros), arr(None), arr(None), arr(bnp), (C.c_int64 * 1)(M), (C.c_int32 * 1)(K),
                                       1e-5, 0.1, stream())
    assert rc == 0
    return bnp[0].double().cpu()


def _forward_problem(B, H, W, Cin, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(K, 3, 3, Cin, generator=g) / (9 * Cin) ** 0.5
    sign = torch.where(torch.rand(Cin, generator=g) < 0.3, -1.0, 1.0)      # some gamma < 0; beta > 0: BN(0) > 0 on most channels
    bn = torch.stack((torch.randn(Cin, generator=g) * 0.5, (torch.rand(Cin, generator=g) + 0.5) * sign, torch.rand(Cin, generator=g) * 0.5 + 0.1,
                      torch.ones(Cin)))
    w64 = w.double().permute(0, 3, 1, 2)
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w64, padding=1).permute(0, 2, 3, 1)
    xa = ((x.double() - bn[0].double()) * bn[1].double() + bn[2].double()).clamp_min(0)
    ypro = F.conv2d(xa.permute(0, 3, 1, 2), w64, padding=1).permute(0, 2, 3, 1)
    return x, w, bn, y, ypro


def _dgrad_problem(B, H, W, Cin, K, seed):
    """Data gradient of a conv Cin -> K (GEMM: reduces over K, Cin columns), with the operands of its fused epilogues."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(K, 3, 3, Cin, generator=g) / (9 * K) ** 0.5
    dy = torch.randn(B, H, W, K, generator=g)
    dx = torch.nn.grad.conv2d_input((B, Cin, H, W), w.double().permute(0, 3, 1, 2), dy.double().permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
    mag = torch.nn.grad.conv2d_input((B, Cin, H, W), w.double().abs().permute(0, 3, 1, 2), dy.double().abs().permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
    bn_y = torch.randn(B, H, W, Cin, generator=g) * 1.5 + 0.3
    mean, invstd = torch.randn(Cin, generator=g) * 0.4, torch.rand(Cin, generator=g) + 0.5
    gamma, beta = torch.rand(Cin, generator=g) + 0.5, torch.randn(Cin, generator=g) * 0.3
    block = torch.stack((mean, gamma * invstd, beta, invstd)).contiguous()
    xhat = (bn_y.double() - mean.double()) * invstd.double()
    bits = torch.rand(B, H, W, Cin, generator=g) > 0.4
    res_src = torch.randn(B, H, W, Cin, generator=g)
    block_out = torch.where(torch.rand(B, H, W, Cin, generator=g) > 0.5, torch.rand(B, H, W, Cin, generator=g) + 0.1, torch.zeros(B, H, W, Cin))
    return dict(w=w, dy=dy, dx=dx, mag=mag, bn_y=bn_y, block=block, xhat=xhat, act=xhat * gamma.double() + beta.double(), bits=bits, res_src=res_src,
                block_out=block_out)


def _sums_err(sums, d, xhat, slack_mask, ref, mag):
    """Error of (sum d, sum d xhat) over the scale of what was added up.  An element of dx carries an error proportional to the
    magnitude of its terms, mag = |dy| (*) |w| (+ |residual|), not to its own value (a pixel's 9 C terms cancel), so the sums are held
    against sum mask mag (x |xhat|): tests/test_gpu_conv_table.py's form, whose scale sum |d| is the same thing once thousands of pixels
    are added and is too small for the one-pixel maps here.  `slack_mask`: elements whose mask may flip."""
    s_ref = torch.stack((d.sum((0, 1, 2)), (d * xhat).sum((0, 1, 2))))
    slack = torch.stack(((ref.abs() * slack_mask).sum((0, 1, 2)), (ref.abs() * xhat.abs() * slack_mask).sum((0, 1, 2))))
    m = mag * (d != 0)
    scale = torch.stack((m.sum((0, 1, 2)), (m * xhat.abs()).sum((0, 1, 2))))
    return float((((sums.double().cpu() - s_ref).abs() - slack).clamp_min(0) / scale.clamp_min(1e-30)).max())


def _run_forward(ops, cv, p, want_family=None):
    from dpft_amd.hip.lib import lib, ptr, stream
    x, w, bn, yref, yref_pro = p
    xg, wg, bng = x.to(DEV), w.to(DEV), bn.to(DEV)
    K, e = w.shape[0], {}
    if want_family:
        ops.profile_start()
    y0, st0 = ops.conv_fwd(cv, xg, wg, want_stats=True)
    if want_family:
        fams = [r[4] for r in ops.profile_collect()]
        assert fams and fams[-1] == want_family, fams
    y1, st1 = ops.conv_fwd(cv, xg, wg, pro=(bng, True), want_stats=True)
    e["fwd"], e["fwd+prologue"] = _rel(y0, yref), _rel(y1, yref_pro)
    ones, zeros = torch.ones(K, device=DEV), torch.zeros(K, device=DEV)
    for st, ref in ((st0, yref), (st1, yref_pro)):      # tile statistics: the 1e-5 form of tests/test_gpu_conv_x3.py
        bnp = ops.bn_finalize(st, cv.tile_rows, cv.M, ones, zeros, 1e-5, 0.1, zeros.clone(), ones.clone())
        yr = ref.reshape(-1, K)
        assert float((bnp[0].double().cpu() - yr.mean(0)).abs().max()) < 1e-5 * float(yr.abs().max())
    # column sums (where the launch carries them)
    acc, used, pused = torch.zeros(4, K, dtype=torch.int64, device=DEV), C.c_int32(-1), C.c_int32(-1)
    y2, st2 = torch.empty_like(y1), torch.empty_like(st1)
    lib.call("dpft_conv2d_nhwc_fwd_sums_f32", C.byref(cv.desc), ptr(xg), ptr(wg), None, ptr(bng), 1, ptr(y2), ptr(st2), ptr(acc),
             C.byref(used), None, None, None, 1, 1e-5, C.byref(pused), ptr(ops.workspace(cv.ws_bytes, xg.device)), stream())
    e["fwd+prologue+sums"] = _rel(y2, yref_pro)
    if used.value == 1:
        yr = yref_pro.reshape(-1, K)
        assert float((_mean_from_sums(acc, cv.M, K) - yr.mean(0)).abs().max()) < 1e-5 * float(yr.abs().max())
    return e


def _run_dgrad(ops, cv, q, fused=True):
    dyg, wt = q["dy"].to(DEV), ops.weight_transpose(q["w"].to(DEV))
    e = {"dgrad": _rel(ops.conv_dgrad(cv, dyg, wt), q["dx"])}
    if not fused:
        return e
    zero = torch.zeros((), dtype=torch.float64)
    bn_y, block = q["bn_y"].to(DEV), q["block"].to(DEV)
    # fused BatchNorm-backward reduction, mask = bn(y) > 0 (unsplit on the smaller tiles: the prefetching kernel, EPF 2)
    sums = torch.zeros(2, cv.C, device=DEV)
    dx, applied = ops.conv_dgrad_bn_reduce(cv, dyg, wt, bn_y, block, sums)
    e["dgrad+bn-reduce"] = _rel(dx, q["dx"])
    if applied:
        d = torch.where(q["act"] > 0, q["dx"], zero)
        assert _sums_err(sums, d, q["xhat"], q["act"].abs() <= 1e-5, q["dx"], q["mag"]) < ABS_BOUND
    # residual + both byte masks + reduction
    ref = q["dx"] + torch.where(q["block_out"] > 0, q["res_src"].double(), zero)
    sums = torch.zeros(2, cv.C, device=DEV)
    dx, applied = ops.conv_dgrad_bn_reduce(cv, dyg, wt, bn_y, block, sums, bn_mask8=_mask8(q["bits"]).to(DEV),
                                           residual=(q["res_src"].to(DEV), q["block_out"].to(DEV), _mask8(q["block_out"] > 0).to(DEV)))
    e["dgrad+residual+mask"] = _rel(dx, ref)
    if applied:
        d = torch.where(q["bits"], ref, zero)
        assert _sums_err(sums, d, q["xhat"], torch.zeros_like(q["bits"]), ref, q["mag"] + q["res_src"].double().abs()) < ABS_BOUND
    return e


def _gate(tag, err):
    """err: {"on" | "off" | "fp32": {form: error}}.  Both split forms below the absolute bound; the row-shared one not above the fp32
    MFMA path's error (its fused forms: against the plain launch of the same operation) times FACTOR."""
    for k_ in err["on"]:
        base = err["fp32"][k_ if k_ in err["fp32"] else ("dgrad" if k_.startswith("dgrad") else "fwd+prologue")]
        print(tag, k_, f"row-shared {err['on'][k_]:.2e}  per-tap {err['off'][k_]:.2e}  fp32 MFMA {base:.2e}")
    for k_ in err["on"]:
        base = err["fp32"][k_ if k_ in err["fp32"] else ("dgrad" if k_.startswith("dgrad") else "fwd+prologue")]
        assert err["off"][k_] < ABS_BOUND, (k_, err["off"][k_])
        assert err["on"][k_] < ABS_BOUND and err["on"][k_] <= base * FACTOR + 1e-9, (k_, base, err["on"][k_])


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "c%d-n%d-split%d" % c)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda s: "x".join(map(str, s)))
def test_row_shared_3x3_forward_and_data_gradient_vs_fp64(geom, cfg, monkeypatch):
    from dpft_amd.hip import ops
    (B, H, W), (Cr, N, splits) = geom, cfg
    seed = 77 + B * 1000 + H * 100 + W * 10 + Cr + N + splits
    p = _forward_problem(B, H, W, Cr, N, seed)      # conv Cr -> N
    q = _dgrad_problem(B, H, W, N, Cr, seed + 1)    # data gradient of a conv N -> Cr: reduces over Cr, N columns
    err = {}
    try:
        for name, row3 in (("off", "0"), ("on", "1")):
            monkeypatch.setenv("DPFT_X3_ROW3", row3)
            monkeypatch.setenv("DPFT_FORCE_TILE", "%s,%d" % (TILE[N], splits))
            ops.conv_set_compute("bf16x3")      # (drops the cached problems: workspace sizes follow the forced split)
            e = _run_forward(ops, ops.conv_problem(B, H, W, Cr, N, 3, 3, 1, 1), p, want_family="x3")
            e.update(_run_dgrad(ops, ops.conv_problem(B, H, W, N, Cr, 3, 3, 1, 1), q))
            err[name] = e
        monkeypatch.delenv("DPFT_FORCE_TILE")
        ops.conv_set_compute("fp32")
        ops.conv_set_split(False)               # the fp32 MFMA kernels
        e = _run_forward(ops, ops.conv_problem(B, H, W, Cr, N, 3, 3, 1, 1), p)
        e.update(_run_dgrad(ops, ops.conv_problem(B, H, W, N, Cr, 3, 3, 1, 1), q, fused=False))
        err["fp32"] = e
    finally:
        ops.conv_set_compute("fp32")
        ops.conv_set_split(True)
    _gate("%s %s" % (geom, cfg), err)


def test_row_shared_residual_data_gradient_with_prefetched_epilogue_vs_fp64(monkeypatch):
    """The residual data gradient whose epilogue operands are fetched during the main loop (EpiPrefetch mode 1) exists only where
    the plan picks it: unsplit, 128 x 64 tiles, at least one workgroup per CU, no forced tile -- 2 x 72 x 57 pixels, 64 -> 256
    columns (2.4 GFLOP: the split rule takes it in the default mode)."""
    from dpft_amd.hip import ops
    B, H, W, Cin, K = 2, 72, 57, 256, 64
    q = _dgrad_problem(B, H, W, Cin, K, 4242)
    err = {}
    try:
        for name, row3 in (("off", "0"), ("on", "1")):
            monkeypatch.setenv("DPFT_X3_ROW3", row3)
            ops.conv_set_split(True)
            err[name] = _run_dgrad(ops, ops.conv_problem(B, H, W, Cin, K, 3, 3, 1, 1), q)
        ops.conv_set_split(False)
        err["fp32"] = _run_dgrad(ops, ops.conv_problem(B, H, W, Cin, K, 3, 3, 1, 1), q, fused=False)
    finally:
        ops.conv_set_split(True)
    _gate("2x72x57 64->256", err)
