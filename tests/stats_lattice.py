"""TEST INFRASTRUCTURE -- the train-mode BatchNorm statistics every conv forward emits, restated on the host in fp64
(tests/test_stats_lattice.py checks this file on the CPU; tests/conv_stats_driver.py runs the kernels against it).

Reference.  Given the exact output y64 (M, K) of a conv and the statistics tile height: the per-tile table (tiles, 2, K) of
(mean, sum of squared deviations), the merged batch statistics, the BN block, the running statistics after one step and the
96-bit fixed-point column sums of common.h (bn_sums_add / bn_sums_get).

Bounds (u = 2^-24; each is derived from the producer's code and the fp64 reference, never from what a kernel returned):

  epilogue (conv_core.h igemm_epilogue -- the pipelined / vector fp32 kernels, the split kernels of conv_x3.hip, the generic
  kernel, with or without the in-launch split-K fix-up) and bn_stats_kernel behind a plain split-K reduction:
      mean = fl(S / cnt) with S the tile's column sum.  The lattice's operands are integers (multiples of 1/2 behind the
      BatchNorm + ReLU prologue), so S is exact in every summation order while sum |y| < 2^24 units: the mean is then ONE
      correctly rounded division -- asserted bit for bit.  Otherwise |dmean| <= (cnt + 1) u sum|y| / cnt.
      M2 = sum fl(fl(y - mean)^2): one rounding in the difference (2 u on the square), one in the square, cnt - 1 in the sum
      of non-negative terms: relative (cnt + 4) u; the rounded mean m' moves the exact sum by cnt (m - m')^2.
  splitk_reduce_stats_kernel: mean = fl(S * fl(1 / cnt)), two roundings: |dmean| <= 2 u (1 + u) |mean|; M2 as above.
  streaming 1x1 kernel (conv_stream.hip): per 32-row block (mb, q) as above, merged into the wave's running pair and then
      over the four waves with Chan's update: each merge rounds dl = mb - mean, nb / nn, their product and the sum --
      |dmean| <= u T (1 + 8 merges) with T = max |y| of the tile (|dl| <= 2 T), merges = rbw - 1 + 3;
      M2: relative (40 + 8 merges) u on the non-negative terms, and the inherited mean error E enters every dl^2:
      4 E sqrt(cnt M2) + 4 cnt E^2 (Cauchy-Schwarz over the merge weights).

A bound that one misplaced row does not exceed would be worthless: wrong_replays() builds the three faults the issue names and
tests/test_stats_lattice.py asserts that check_table() flags each of them for every ragged launch of the GPU test."""
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

from tests import conv_lattice as L

U = 2.0 ** -24
NUM_CU = 256                      # host_consts.h: kNumCU
BKV, BK = 64, 32                  # conv_plan.h
SK_FIXUP_DEFAULT = 7              # DPFT_SK_FIXUP


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------------
# the fp64 reference
# ---------------------------------------------------------------------------------------------------------------------------------
def tile_counts(M, tile_rows):
    tiles = cdiv(M, tile_rows)
    return np.array([min(tile_rows, M - t * tile_rows) for t in range(tiles)], dtype=np.int64)


def tile_table(y64, tile_rows):
    """(tiles, 2, K) float64: tile t covers rows [t * tile_rows, min((t + 1) * tile_rows, M)); mean and sum of squared deviations."""
    y = np.asarray(y64, dtype=np.float64)
    M, K = y.shape
    out = np.empty((cdiv(M, tile_rows), 2, K))
    for t in range(out.shape[0]):
        blk = y[t * tile_rows:(t + 1) * tile_rows]
        out[t, 0] = blk.mean(0)
        out[t, 1] = ((blk - out[t, 0]) ** 2).sum(0)
    return out


def merge_table(table, counts):
    """Batch (mean, M2) of a per-tile table in fp64 (the exact algebra of Chan's merge)."""
    n = counts.astype(np.float64)[:, None]
    N = n.sum()
    mean = (n * table[:, 0]).sum(0) / N
    m2 = (table[:, 1] + n * (table[:, 0] - mean) ** 2).sum(0)
    return mean, m2


def merged(y64):
    """batch mean and BIASED variance of y64 (M, K)."""
    y = np.asarray(y64, dtype=np.float64)
    mean = y.mean(0)
    return mean, ((y - mean) ** 2).mean(0)


def bn_block(mean, var, gamma, beta, eps):
    """(4, K): mean, gamma * invstd, beta, invstd."""
    invstd = 1.0 / np.sqrt(var + eps)
    return np.stack([mean, np.asarray(gamma, np.float64) * invstd, np.asarray(beta, np.float64), invstd])


def running_after(mean, var, M, rm, rv, momentum):
    """Running statistics after one step: (1 - m) r + m stat with the unbiased variance var * M / (M - 1); at M == 1 the
    kernels keep the biased one (bn_finalize_kernel, bn_finalize_sums_multi_kernel)."""
    unbiased = var * (M / (M - 1.0)) if M > 1 else var
    return (1.0 - momentum) * np.asarray(rm, np.float64) + momentum * mean, (1.0 - momentum) * np.asarray(rv, np.float64) + momentum * unbiased


# ---------------------------------------------------------------------------------------------------------------------------------
# the fixed-point column sums (common.h): floor(s / 4) to the high word, (s - 4 high) 2^46 truncated to the low word, integer adds
# ---------------------------------------------------------------------------------------------------------------------------------
def encode_units(s):
    """fp64 array -> object array of Python ints: the addend bn_sums_add makes of s, in units of 2^-46 (high * 2^48 + low).
    Every step of the rule is exact in fp64 but the truncation, which is restated here."""
    s = np.asarray(s, dtype=np.float64)
    h = np.floor(s * 0.25)
    lo = np.trunc((s - h * 4.0) * 2.0 ** 46)
    assert bool((lo >= 0).all()) and bool((lo < 2.0 ** 48).all())
    return np.array([int(a) * (1 << 48) + int(b) for a, b in zip(h.ravel(), lo.ravel())], dtype=object).reshape(s.shape)


def encode_words(s1, s2):
    """[4][K] int64 words of ONE addend per channel (as bn_lattice.encode_sums, with the truncation)."""
    words = []
    for s in (s1, s2):
        s = np.asarray(s, dtype=np.float64)
        h = np.floor(s * 0.25)
        words += [h.astype(np.int64), np.trunc((s - h * 4.0) * 2.0 ** 46).astype(np.int64)]
    return np.stack(words)


def decode_units(words):
    """(4, K) int64 words -> two object arrays of Python ints in units of 2^-46 (bn_sums_get, exactly)."""
    w = np.asarray(words, dtype=np.int64)
    return tuple(np.array([int(h) * (1 << 48) + int(lo) for h, lo in zip(w[2 * i], w[2 * i + 1])], dtype=object) for i in range(2))


def sums_addends(table32, counts):
    """What a launch adds per tile: s1 = cnt mean (exact in fp64), s2 = M2 + cnt mean^2 from the fp32 table it would write."""
    t = np.asarray(table32, dtype=np.float32).astype(np.float64)
    n = counts.astype(np.float64)[:, None]
    return n * t[:, 0], t[:, 1] + n * t[:, 0] * t[:, 0]


def sums_expected(table32, counts):
    """-> (units1, units2, slack2): the accumulated units of both sums and the bound on sum 2 in units.  Sum 1 is exact: cnt mean
    is exact in fp64 and so is its encoding up to the truncation restated above.  Sum 2 per addend: the 2^-46 truncation (one
    unit) and the fp64 rounding of M2 + cnt mean^2 -- two roundings unfused, one fused, so the value may differ from this
    restatement by two ulp."""
    s1, s2 = sums_addends(table32, counts)
    u1, u2 = encode_units(s1).sum(0), encode_units(s2).sum(0)
    ulp = np.spacing(np.abs(s2).max(0)) * 2.0 ** 46
    slack = [int(math.ceil(len(counts) * (1 + 2 * float(v)))) for v in ulp]
    return u1, u2, slack


def block_from_units(u1, u2, M, gamma, beta, eps):
    """BN block and (mean, biased var) from decoded sums, in exact rational arithmetic up to the square root."""
    mean = [Fraction(int(a), 1 << 46) / M for a in u1]
    var = [max(Fraction(int(b), 1 << 46) / M - m * m, Fraction(0)) for b, m in zip(u2, mean)]
    mean, var = np.array([float(m) for m in mean]), np.array([float(v) for v in var])
    return bn_block(mean, var, gamma, beta, eps), mean, var


# ---------------------------------------------------------------------------------------------------------------------------------
# the bounds, and the check of a table against them
# ---------------------------------------------------------------------------------------------------------------------------------
FORMS = ("epilogue", "reduce_stats", "stream")
TableRef = namedtuple("TableRef", "form counts table exact mean32 mean_bound m2_bound")


def table_reference(y64, tile_rows, form, unit=1.0, rbw=1):
    """The fp64 table of y64 (M, K) and the bounds of ``form`` (module docstring).  ``unit``: the grid y lies on (1, or 1/2 behind
    the prologue); ``rbw``: row blocks per wave of the streaming kernel."""
    assert form in FORMS
    y = np.asarray(y64, dtype=np.float64)
    M, K = y.shape
    assert bool((np.round(y / unit) * unit == y).all())
    counts = tile_counts(M, tile_rows)
    table = tile_table(y, tile_rows)
    tiles = len(counts)
    A = np.stack([np.abs(y[t * tile_rows:(t + 1) * tile_rows]).sum(0) for t in range(tiles)])
    T = np.stack([np.abs(y[t * tile_rows:(t + 1) * tile_rows]).max(0) for t in range(tiles)])
    S = np.stack([y[t * tile_rows:(t + 1) * tile_rows].sum(0) for t in range(tiles)])
    n = counts.astype(np.float64)[:, None]
    mean, m2 = table[:, 0], table[:, 1]
    exact_sum = A < 2.0 ** 24 * unit
    mean32 = (S.astype(np.float32) / counts.astype(np.float32)[:, None]).astype(np.float32)      # one IEEE division
    merges = rbw - 1 + 3
    if form == "epilogue":
        exact = exact_sum
        e_m = np.where(exact_sum, U * np.abs(mean), (n + 1) * U * A / n)
    elif form == "reduce_stats":
        exact = np.zeros_like(exact_sum)
        e_m = np.where(exact_sum, 2 * U * (1 + U) * np.abs(mean), (n + 2) * U * A / n)
    else:
        exact = np.zeros_like(exact_sum)
        e_m = U * T * (1 + 8 * merges)
    if form == "stream":
        e_m2 = (40 + 8 * merges) * U * m2 + 4 * e_m * np.sqrt(n * m2) + 4 * n * e_m ** 2
    else:
        e_m2 = (n + 4) * U * (m2 + n * e_m ** 2) + n * e_m ** 2
    return TableRef(form, counts, table, exact, mean32, e_m, e_m2)


def check_table(got32, ref):
    """-> (violations, ratios): every entry of the fp32 table (tiles, 2, K) against ``ref``; ratios = worst |error| / bound of the
    bounded means and of M2 (0 where every mean is compared bit for bit)."""
    g = np.ascontiguousarray(got32)
    assert g.dtype == np.float32 and g.shape == ref.table.shape, (g.dtype, g.shape, ref.table.shape)
    bad = []
    if not bool(np.isfinite(g).all()):
        bad.append(f"{int((~np.isfinite(g)).sum())} entries are not finite")
        g = np.nan_to_num(g, nan=1e30, posinf=1e30, neginf=-1e30)
    g_mean = np.ascontiguousarray(g[:, 0])
    gm, gq = g_mean.astype(np.float64), g[:, 1].astype(np.float64)
    wrong = ref.exact & (g_mean.view(np.int32) != ref.mean32.view(np.int32)) & ~((g_mean == 0) & (ref.mean32 == 0))
    if wrong.any():
        t, c = np.argwhere(wrong)[0]
        bad.append(f"mean: {int(wrong.sum())} entries differ from fl(S / cnt), first tile {t} channel {c}: {g_mean[t, c]!r} vs {ref.mean32[t, c]!r}")
    dm = np.abs(gm - ref.table[:, 0])
    over = ~ref.exact & (dm > ref.mean_bound)
    if over.any():
        t, c = np.argwhere(over)[0]
        bad.append(f"mean: {int(over.sum())} entries beyond the bound, first tile {t} channel {c}: |d| {dm[t, c]:.3e} > {ref.mean_bound[t, c]:.3e}")
    dq = np.abs(gq - ref.table[:, 1])
    over = dq > ref.m2_bound
    if over.any():
        t, c = np.argwhere(over)[0]
        bad.append(f"M2: {int(over.sum())} entries beyond the bound, first tile {t} channel {c}: |d| {dq[t, c]:.3e} > {ref.m2_bound[t, c]:.3e} (M2 {ref.table[t, 1, c]:.6g})")
    free = ~ref.exact & (ref.mean_bound > 0)
    r_mean = float((dm[free] / ref.mean_bound[free]).max()) if free.any() else 0.0
    pos = ref.m2_bound > 0
    r_m2 = float((dq[pos] / ref.m2_bound[pos]).max()) if pos.any() else 0.0
    return bad, (r_mean, r_m2)


def faithful_replay(y64, tile_rows):
    """The table a correct epilogue writes, up to the order of its M2 sum: fp32 mean by one division, M2 about THAT mean."""
    y = np.asarray(y64, dtype=np.float64)
    counts = tile_counts(y.shape[0], tile_rows)
    out = np.empty((len(counts), 2, y.shape[1]), dtype=np.float32)
    for t, n in enumerate(counts):
        blk = y[t * tile_rows:t * tile_rows + n]
        out[t, 0] = blk.sum(0).astype(np.float32) / np.float32(n)
        out[t, 1] = ((blk - out[t, 0].astype(np.float64)) ** 2).sum(0)
    return out


def wrong_replays(y64, tile_rows):
    """dict name -> fp32 table of a deliberately WRONG producer (the faults of the issue); only what applies to the geometry:
    'row moved' needs two tiles, the two others a ragged last tile."""
    y = np.asarray(y64, dtype=np.float64)
    M = y.shape[0]
    counts = tile_counts(M, tile_rows)
    good = faithful_replay(y, tile_rows)
    out = {}

    def pair(rows, div=None, extra_zero=False):
        n = len(rows) + (1 if extra_zero else 0)
        mean = (rows.sum(0) / (div if div else n)).astype(np.float32)
        q = ((rows - mean.astype(np.float64)) ** 2).sum(0) + (mean.astype(np.float64) ** 2 if extra_zero else 0.0)
        return mean, q.astype(np.float32)
    if len(counts) >= 2:      # the last row of tile 0 counted into tile 1
        t = good.copy()
        t[0, 0], t[0, 1] = pair(y[:tile_rows - 1])
        t[1, 0], t[1, 1] = pair(y[tile_rows - 1:tile_rows + counts[1]])
        out["row moved"] = t
    if M % tile_rows:
        last = y[(len(counts) - 1) * tile_rows:]
        t = good.copy()
        t[-1, 0], t[-1, 1] = pair(last, div=tile_rows)
        out["last tile / tile_rows"] = t
        t = good.copy()
        t[-1, 0], t[-1, 1] = pair(last, extra_zero=True)
        out["padded row counted"] = t
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the launch plan of a forward conv with statistics, restated from conv_plan.h (plan_igemm / choose_tile, kind = kFwd)
# ---------------------------------------------------------------------------------------------------------------------------------
Plan = namedtuple("Plan", "kernel bm bn splits split_kind stat_sums pro_from_sums stream_unfit rbw")
# kernel: stream | generic | pipe | x3 | vec; split_kind: unsplit | fixup | reduce_stats | reduce_plain


def stream_rows(c, mode):
    """Tile rows of the streaming 1x1 kernel where stream1x1_match takes the shape, else 0."""
    if L.MODES[mode][0] == "bf16" or (c.kh, c.kw, c.stride, c.pad) != (1, 1, 1, 0) or c.C not in (64, 128) or c.K % 256:
        return 0
    M = L.rows(c)
    if M < 4096 or (M // 32) * (c.K // 256) < 2 * NUM_CU or M * max(c.C, c.K) >= 2 ** 31:
        return 0
    return 32 * 4 * max(1, cdiv(cdiv(M, 32), 4 * 2048))


def plan_fwd(c, mode, tile=None, pro=False, bias=False, sums=False, sk_fixup=SK_FIXUP_DEFAULT):
    """``pro``: the BatchNorm + ReLU prologue; statistics wanted."""
    compute, split_on = L.MODES[mode]
    M, N = L.rows(c), c.K
    taps = c.kh * c.kw
    vec = c.C % BKV == 0
    ksteps = taps * c.C // BKV if vec else cdiv(taps * c.C, BK)
    sr = stream_rows(c, mode)
    if sr and not bias:
        return Plan("stream", sr, 256, 1, "unsplit", sums and M < 2 ** 22, True, False, sr // 128)
    if not vec:
        return Plan("generic", 128, 32 if N <= 32 else 64, 1, "unsplit", False, False, bool(sr), 0)
    multi = not (taps == 1 and c.stride == 1)
    assert not (split_on and multi and tile is None and 2.0 * M * N * ksteps * BKV >= 2e9), "the automatic split-kernel tiles are not restated"
    if tile is not None:
        bm, bn, splits = tile[0], tile[1], max(tile[2], 1)
        while splits > 1 and ksteps // splits < 2:
            splits -= 1
    else:
        best, bm, bn = -1.0, 64, 64
        for (cm, cn), eff in zip(((128, 128), (128, 64), (64, 64)), (1.0, 0.92, 0.80)):
            if cn > 64 and N <= 64:
                continue
            nwg = cdiv(M, cm) * cdiv(N, cn)
            waves = nwg / (NUM_CU * 2)
            score = eff * (waves / math.ceil(waves)) * (M * N / (cdiv(M, cm) * cm * cdiv(N, cn) * cn))
            if score > best:
                best, bm, bn = score, cm, cn
        nwg = cdiv(M, bm) * cdiv(N, bn)
        splits = 1
        if nwg < NUM_CU and ksteps >= 8 and not (nwg >= 200 and ksteps <= 32):
            splits = min(16, (NUM_CU * 2 + nwg - 1) // nwg)
            while splits > 1 and ksteps // splits < 4:
                splits -= 1
    fixup = bool(sk_fixup & 1) and splits > 1 and N % 4 == 0 and splits * M * N * 4 < 2 ** 31
    if splits == 1:
        kind = "unsplit"
    elif fixup:
        kind = "fixup"
    else:
        kind = "reduce_stats" if (not bias and N % 64 == 0 and bm <= 128) else "reduce_plain"
    pipe = compute != "bf16"
    x3_tile = (bm, bn) in ((128, 128), (128, 64), (64, 64))
    if compute == "bf16x3" and tile is not None and x3_tile:
        kernel = "x3"
    else:
        kernel = "pipe" if pipe else "vec"
    if bm == 64 and bn == 128 and not pipe:
        bn = 64
    stat_sums = sums and not bias and N % 4 == 0 and kind in ("unsplit", "fixup") and M < 2 ** 22
    return Plan(kernel, bm, bn, splits, kind, stat_sums, kernel in ("x3", "pipe") and pro and 12 * c.C <= 16384, bool(sr), 0)


def table_form(plan):
    """Which bound the table of a planned launch gets."""
    if plan.kernel == "stream":
        return "stream"
    return "reduce_stats" if plan.split_kind == "reduce_stats" else "epilogue"      # (reduce_plain: bn_stats_kernel, the epilogue's arithmetic)


def form_name(plan):
    return f"{plan.kernel}/{plan.split_kind}"


# ---------------------------------------------------------------------------------------------------------------------------------
# the launches of tests/test_gpu_conv_stats.py
# ---------------------------------------------------------------------------------------------------------------------------------
# small cases of the vector path (the one large case of conv_lattice.C64 is not needed by any form)
C64 = [c for c in L.C64 if c.name not in L.LARGE_NAMES]
# the generic kernel: a stem-shaped C = 3 case (below the stem matcher's size), generic-class and C % 64 == 32 cases
GENERIC = [L.make_case("stats-stem-small", 2, 21, 27, 3, 64, 7, 7, 2, 3)] + [L.by_name(n) for n in ("rc-5x3-generic", "s3-2x7-generic", "c96-k64-3x3")]
# the streaming 1x1 kernel at its smallest maps: M >= 4096 and (M / 32) (K / 256) >= 512.  M = 4160 = 32.5 workgroups of 128 rows
# (the last one has two idle waves), M = 4209 is no multiple of 32 either
STREAM = [L.make_case("stats-stream-c64-m4160", 1, 65, 64, 64, 1024, 1, 1, 1, 0),
          L.make_case("stats-stream-c64-m4209", 1, 61, 69, 64, 1024, 1, 1, 1, 0),
          L.make_case("stats-stream-c128-m4209", 1, 69, 61, 128, 1024, 1, 1, 1, 0)]
EXTRA = {c.name: c for c in GENERIC + STREAM}
Launch = namedtuple("Launch", "case mode tile pro")
# (mode, forced tile) groups of the vector path; every FORCE_TILES entry in fp32 and in bf16x3 mode (there the x3 tiles go to
# the split kernels), the unforced plan in every mode
GROUPS = [(m, None) for m in L.MODES] + [(m, t) for m in ("fp32", "bf16x3") for t in L.FORCE_TILES]
# the separate reduction launches exist behind DPFT_SK_FIXUP=0 only (read once per process): a child process runs these
CHILD_GROUPS = [("fp32", "128,64,2"), ("fp32", "64,64,3")]
REQUIRED_FORMS = ("pipe/unsplit", "pipe/fixup", "pipe/reduce_plain", "x3/unsplit", "x3/fixup", "vec/unsplit", "vec/fixup",
                  "generic/unsplit", "stream/unsplit")
REQUIRED_CHILD_FORMS = ("pipe/reduce_stats", "pipe/reduce_plain")


def case_by_name(name):
    return EXTRA[name] if name in EXTRA else L.by_name(name)


def parse_tile(tile):
    return None if tile is None else tuple(int(v) for v in tile.split(","))


def group_launches(mode, tile):
    return [Launch(c, mode, tile, pro) for c in C64 for pro in (False, True)]


def other_launches():
    out = [Launch(c, m, None, False) for c in GENERIC for m in ("fp32", "bf16")]
    return out + [Launch(c, m, None, pro) for c in STREAM for m in ("fp32", "fp32+split") for pro in (False, True)]


def all_launches(child=False):
    if child:
        return [l for g in CHILD_GROUPS for l in group_launches(*g)]
    return [l for g in GROUPS for l in group_launches(*g)] + other_launches()


def launch_plan(l, sums=False, bias=False, child=False):
    return plan_fwd(l.case, l.mode, parse_tile(l.tile), l.pro, bias=bias, sums=sums, sk_fixup=0 if child else SK_FIXUP_DEFAULT)


def forms_reached(child=False):
    return {form_name(launch_plan(l, child=child)) for l in all_launches(child)}


_y = {}


def case_output(c, pro):
    """(y64 as a (M, K) numpy array, unit of its grid, the operands) -- computed once per (case, prologue)."""
    key = (c.name, pro)
    if key not in _y:
        o = L.operands(c)
        y = L.reference(c, o, pro=pro)["y"].reshape(-1, c.K).numpy()
        _y[key] = (y, 0.5 if pro else 1.0, o)
    return _y[key]


def launch_reference(l, child=False):
    p = launch_plan(l, child=child)
    y, unit, _ = case_output(l.case, l.pro)
    return p, table_reference(y, p.bm, table_form(p), unit, max(p.rbw, 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# bn_stats_kernel / bn_finalize_kernel called directly (tests/test_gpu_bn_stats.py)
# ---------------------------------------------------------------------------------------------------------------------------------
# (M, K, tile_rows).  Exact tier: M and every tile count a power of two, M <= 4096
EXACT_CASES = [(1, 12, 64), (32, 64, 64), (64, 96, 64), (2048, 256, 64), (4096, 320, 64), (128, 2048, 128), (4096, 64, 128),
               (256, 320, 256), (512, 12, 256), (2, 2048, 256), (1, 320, 128), (2048, 96, 256)]
# float tier: tiles 1, 32, 33, 65; ragged last tiles (one of a single row); M < tile_rows; M == 1
FLOAT_CASES = [(1, 12, 64), (37, 96, 128), (2048, 64, 64), (2053, 320, 64), (8269, 256, 128), (8193, 12, 256), (300, 2048, 128),
               (16640, 96, 256), (129, 64, 128)]


def exact_data(M, K, tile_rows, seed=0):
    """Integers in [-7, 7] whose tile means are quarter-integers mu + j / 4 (mu per channel, j per tile): rows come in pairs
    (mu + a, mu - a), |a| <= 3, |mu| <= 3, and cnt j / 4 rows get + 1.  Deviations then have two fractional bits, their squares
    four, and every partial sum of either kernel stays below 2^24 units of its grid: the table, the merged mean, M2 = S2 - S1^2 / M
    and the variance are exact in fp32 in every summation order (S1 = M (mean - pivot) is an integer below 3 M / 4 <= 3072)."""
    assert M & (M - 1) == 0 and M <= 4096 and (M <= tile_rows or M % tile_rows == 0)
    g = np.random.default_rng(1000 * seed + 7 * M + 3 * K + tile_rows)
    mu = g.integers(-3, 4, size=K)
    y = np.empty((M, K), dtype=np.float64)
    for t, n in enumerate(tile_counts(M, tile_rows)):
        n = int(n)
        blk = np.tile(mu, (n, 1)).astype(np.float64)
        if n > 1:
            a = g.integers(-3, 4, size=(n // 2, K))
            blk[0::2] += a
            blk[1::2] -= a
        if n % 4 == 0:
            j = g.integers(0, 4, size=K)
            order = np.argsort(g.random((n, K)), axis=0)      # a random permutation of the rows per channel
            blk += order < (n // 4 * j)[None, :]
        y[t * tile_rows:t * tile_rows + n] = blk
    assert float(np.abs(y).max()) <= 7
    return y


def float_data(M, K, seed=0):
    """Gaussian columns with a per-channel scale and an offset of up to 200 standard deviations (the stem's raw 0..255 inputs)."""
    g = np.random.default_rng(2000 * seed + 11 * M + K)
    sigma = g.uniform(0.5, 2.0, size=K)
    off = g.uniform(-200.0, 200.0, size=K) * sigma
    return (g.standard_normal((M, K)) * sigma + off).astype(np.float32)


def bn_stats_bounds(y32, tile_rows):
    """bn_stats_kernel on float data: groups = 256 / min(K, 256) threads share a column, each sums every groups-th row in order,
    then the groups partials are added in order: chain = ceil(cnt / groups) + groups roundings, + 1 for the division.
    -> (fp64 table, mean bound, M2 bound)."""
    y = np.asarray(y32, dtype=np.float32).astype(np.float64)
    M, K = y.shape
    groups = 256 // min(K, 256)
    counts = tile_counts(M, tile_rows)
    table = tile_table(y, tile_rows)
    A = np.stack([np.abs(y[t * tile_rows:(t + 1) * tile_rows]).sum(0) for t in range(len(counts))])
    n = counts.astype(np.float64)[:, None]
    chain = np.ceil(n / groups) + groups
    e_m = (chain + 1) * U * A / n
    e_m2 = (chain + 3) * U * (table[:, 1] + n * e_m ** 2) + n * e_m ** 2
    return table, e_m, e_m2


def finalize_bounds(table32, counts, M, gamma, eps, momentum, rm, rv):
    """bn_finalize_kernel against the fp64 merge of the fp32 table it reads.  With d_t = mean_t - pivot (one rounding) and L =
    ceil(tiles / 32) + 32 the longest chain of additions:  S1 = sum cnt d within (L + 2) u sum cnt |d|;  S2 = sum (M2_t + cnt d^2)
    of non-negative terms within (L + 4) u S2;  mean = fma(S1, 1 / M, pivot): the errors of S1 and 1 / M over M plus one rounding
    of the mean;  M2 = S2 - S1^2 / M;  invstd = 1 / sqrtf(var + eps): half the relative error of var + eps plus three roundings.
    -> dict of (fp64 reference, bound): mean, invstd, scale, rm, rv."""
    t = np.asarray(table32, dtype=np.float32).astype(np.float64)
    n = counts.astype(np.float64)[:, None]
    tiles = len(counts)
    Lc = math.ceil(tiles / 32) + 32
    pivot = t[0, 0]
    d = t[:, 0] - pivot
    s1, s1_abs = (n * d).sum(0), (n * np.abs(d)).sum(0) * (1 + U)
    s2 = (t[:, 1] + n * d * d).sum(0)
    mean, m2 = merge_table(t, counts)
    e_s1 = (Lc + 2) * U * s1_abs
    e_mean = e_s1 / M + 2 * U * np.abs(s1) / M + U * np.abs(mean) * (1 + 2 * U)
    e_m2 = (Lc + 4) * U * s2 + (2 * e_s1 * np.abs(s1) + e_s1 ** 2 + 4 * U * s1 * s1) / M + U * m2
    var = m2 / M
    e_var = e_m2 / M + 2 * U * var
    invstd = 1.0 / np.sqrt(var + eps)
    e_invstd = invstd * (0.5 * (e_var + U * (var + eps)) / (var + eps) + 3 * U)
    scale = np.asarray(gamma, np.float64) * invstd
    e_scale = np.abs(np.asarray(gamma, np.float64)) * e_invstd + U * np.abs(scale)
    unb = m2 / (M - 1) if M > 1 else var
    e_unb = (e_m2 / (M - 1) if M > 1 else e_var) + U * unb
    rm, rv = np.asarray(rm, np.float64), np.asarray(rv, np.float64)
    rm_new, rv_new = (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * unb
    e_rm = momentum * e_mean + 4 * U * (np.abs((1 - momentum) * rm) + np.abs(momentum * mean))
    e_rv = momentum * e_unb + 4 * U * (np.abs((1 - momentum) * rv) + np.abs(momentum * unb))
    return dict(mean=(mean, e_mean), invstd=(invstd, e_invstd), scale=(scale, e_scale), rm=(rm_new, e_rm), rv=(rv_new, e_rv))


def sums_finalize_bounds(u1, u2, M, gamma, beta, eps, momentum, rm, rv):
    """bn_finalize_sums_multi_kernel (bn_from_sums) against the exact rational value of the decoded sums: m and var are fp64
    expressions (var = S2 / M - m^2 cancels: 4 ulp of S2 / M), mean = (float)m is one rounding (two where the fp64 value sits on a
    tie), invstd = 1 / sqrtf((float)var + eps) four roundings at half weight for those under the root."""
    block, mean, var = block_from_units(u1, u2, M, gamma, beta, eps)
    s2m = np.array([float(Fraction(int(b), 1 << 46) / M) for b in u2])
    e_var = 4 * 2.0 ** -53 * s2m + U * var
    e_mean = U * np.abs(mean) * (1 + 2.0 ** -20)
    invstd = block[3]
    e_invstd = invstd * (0.5 * (e_var + U * (var + eps)) / (var + eps) + 3 * U)
    e_scale = np.abs(np.asarray(gamma, np.float64)) * e_invstd + U * np.abs(block[1])
    unb = var * (M / (M - 1.0)) if M > 1 else var
    e_unb = e_var * (M / (M - 1.0) if M > 1 else 1.0) + 2 * U * unb
    rm, rv = np.asarray(rm, np.float64), np.asarray(rv, np.float64)
    rm_new, rv_new = (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * unb
    e_rm = momentum * e_mean + 4 * U * (np.abs((1 - momentum) * rm) + np.abs(momentum * mean))
    e_rv = momentum * e_unb + 4 * U * (np.abs((1 - momentum) * rv) + np.abs(momentum * unb))
    return dict(mean=(mean, e_mean), invstd=(invstd, e_invstd), scale=(block[1], e_scale), rm=(rm_new, e_rm), rv=(rv_new, e_rv))
