"""The BatchNorm passes of dpft_amd/csrc/bn.hip off the model's shapes: cases, fp64 reference and a restatement of the host dispatch
(CPU only; the GPU half is tests/bn_passes_driver.py, run by tests/test_gpu_bn_passes.py).

Passes: act (out = [relu](bn(y) [+ bn_r(res) | + res]), optional fp32 copy and mask byte), backward reduce and apply (three mask
sources, train and frozen), the stem's 3 x 3 / stride 2 / pad 1 max-pool and its backward, add and the fp32 -> bf16 conversion.

Two value tiers.

EXACT.  Operands are small integers and dyadic fractions: y, res in [-3, 3], dout in [-2, 2], mean in [-1, 1], invstd in
{1/2, 1, 2}, gamma in {+-1/2, +-1}, beta in {-1 .. 1} by halves, sums / M in {0, +-1/2, +-1} and {0, +-1/2}.  Every intermediate of
every kernel expression -- the generic  ga is (d - s0/M - xhat s1/M)  and the fixed-channel  A d + (Q (y - mu) + P),  P = -A s0/M
-- is then a dyadic number of fewer than 24 bits and every stored value one of at most 8 (bf16), so the GPU result has to equal
fp64 bit for bit whatever the order of the operations and whether or not the compiler fuses a multiply into an add.
exact_proof() replays the expressions in numpy float32 (rounded after every operation AND with the products kept unrounded
inside an add, as a fused multiply-add does) and asserts equality with fp64.  The one inexact operand is 1/M: the train-mode
apply carries sums = M * a only where fl(M a * fl(1/M)) == a holds AND the fused replay agrees, i.e. in practice for M a power
of two; elsewhere the sums are zero (the case keeps every other check, and the frozen form, exact for every M, runs everywhere).
Reduce sums are halves below 2^23 in absolute sum, so the order of the atomics cannot matter.

FLOAT.  Gaussian data with channels of |mean| / std in {1, 30, 1000} and invstd from 1e-3 to 1e3; per element the error must stay
under  c u T,  T = the sum of the magnitudes of the terms of the DEFINING expression, u = 2^-24, plus, for bf16 storage, one rounding
of the result to 8 significant bits: half a unit in the last place of the reference, 2^-8 * 2^floor(log2 |ref|) -- between 2^-9
and 2^-8 of the value, nothing given away near the top of a binade.
Derivation of c by counting roundings, each at most u relative to the term it touches.  Generic apply,
ga is (d - s0 invM - xhat s1 invM): xhat = (y - mu) is: 2; xhat s1: 3; times invM: 4, invM = fl(1/M) itself: 5; the second
subtraction rounds once: 6; A = ga is: 7; the outer product: 8 on the third term (6 and 4 on the other two).  Fixed-channel apply,
A d + (Q (y - mu) + P): Q = -A is (s1 invM): A (1), A is (2), s1 invM (1 + 1 for invM), their product: 5; y - mu: 6; the inner fma
rounds once: 7; the outer fma once more: 8 (P = -A (s0 invM): 4, + 2 = 6).  Both forms: c = 8.  act: (y - mu) 1, fma 1, the same 2 for
the residual's BatchNorm, the add 1: 5 <= 8; one constant for all passes.
T is taken from the defining expression (|ga is d| + |ga is s0/M| + |ga is xhat s1/M|), NOT from terms like |Q y| and |Q mu| of a
rearranged one, which cancel when |mean| >> std: that cancellation is what the tier is there to see.

FOUND AND FIXED.  The fixed-channel apply kernels used to fold Q mu into P and compute A d + (Q y + P): the roundings are then
relative to |Q y| and |Q mu|, which exceed |Q (y - mu)| by |mean| / std -- and by more wherever y is near the mean.  The float32
replay of that expression (form 'fixc-uncentred', kept for the record and asserted to miss) exceeds the halved bound up to 10 x
at |mean| / std = 1, 130 x at 30 and 18 000 x at 1000; on an MI355X bn_bwd_apply_fixc_kernel<2> reached 1.08 x the full bound at
|mean| / std = 1, 10 - 75 x at 30 and 750 - 4500 x at 1000 (K = 32, 64, 2048) while every other kernel stayed below 1.  The kernels
now centre y before the multiply ("BatchNorm pass lattice").
"""
import collections
import math

import numpy as np
import torch

NUM_CU = 256                      # common.h: kNumCU
PB_TH, PB_TW, PB_CQ = 4, 8, 8     # bn.hip: windows per tile (rows, cols), channel quads per tile
DEFAULT_SWITCHES = dict(fixc=2, wide16=1, fat=1, tiled=1, per_cu=8)
SWITCH_ENV = dict(fixc="DPFT_BN_FIXC", wide16="DPFT_BN_WIDE16", fat="DPFT_BN_FAT", tiled="DPFT_POOL_BWD_TILED",
                  per_cu="DPFT_EW_BLOCKS_PER_CU")
# the child processes of tests/test_gpu_bn_passes.py: one switch changed each
SWITCH_RUNS = [dict(fixc=0), dict(fixc=1), dict(fixc=3), dict(wide16=0), dict(fat=0), dict(tiled=0), dict(per_cu=1)]
C_BOUND = 8.0
U32, U16 = 2.0 ** -24, 2.0 ** -8


def switches(**changed):
    sw = dict(DEFAULT_SWITCHES)
    sw.update(changed)
    return sw


def switches_from_env(env):
    return switches(**{k: int(env[v]) for k, v in SWITCH_ENV.items() if v in env})


# ---------------------------------------------------------------------------------------------------------------------------------
# the host dispatch of bn.hip, restated (coverage accounting; the GPU test compares every verdict with dpft_bn_last_form)
# ---------------------------------------------------------------------------------------------------------------------------------
def ew_blocks(items, sw):
    return max(1, min((items + 255) // 256, NUM_CU * sw["per_cu"]))


def fixc_grid(kq, items, blocks, sw):
    """-> (fixed-channel form possible, block count): bn.hip fixc_grid (the 16-byte bf16 forms)."""
    if sw["fixc"] <= 0 or items < 4096 or items >= 1 << 30 or kq <= 0:
        return False, blocks
    if 256 % kq == 0:
        return True, blocks
    if kq % 256 != 0:
        return False, blocks
    f = kq // 256
    if blocks < f:
        return False, blocks
    return True, blocks - blocks % f


def f32_fixc(M, K, sw, out32=False):
    """-> (ok, blocks, f): the fp32 rule shared by bn_act_any, bn_act_sums and bn_bwd_apply_zeroing."""
    n4, K4 = M * K // 4, K // 4
    blocks = ew_blocks((n4 + 1) // 2 if sw["fat"] and sw["fixc"] >= 2 else n4, sw)
    ok = sw["fixc"] > 0 and not out32 and 4096 <= n4 < 1 << 30
    f = 1
    if ok and 256 % K4 != 0:
        f = K4 // 256
        ok = K4 % 256 == 0 and blocks >= f
        if ok:
            blocks -= blocks % f
    return ok, (blocks if ok else ew_blocks(n4, sw)), f


Launch = collections.namedtuple("Launch", "form blocks per_thread trips trimmed")


def _trips(items, blocks, per_thread):
    return -(-items // (blocks * 256 * per_thread))


def elementwise_launch(kind, M, K, bf16, sw, out32=False):
    """The launch of an act / apply pass: kernel form (ops.BN_FORMS), grid, quads (or octets) per thread and trip, the largest
    number of trips a thread makes, whether `blocks -= blocks % f` removed a block."""
    n4 = M * K // 4
    if bf16 and sw["wide16"] and K % 8 == 0:                       # (the tests' tensors are 16-byte aligned)
        n8 = n4 // 2
        b0 = ew_blocks(n8, sw)
        ok, blocks = fixc_grid(K // 8, n8, b0, sw)
        return Launch("wide16_fixc" if ok else "wide16", blocks if ok else b0, 2, _trips(n8, blocks if ok else b0, 2), ok and blocks != b0)
    if bf16:
        b = ew_blocks(n4, sw)
        return Launch("generic", b, 2, _trips(n4, b, 2), False)
    ok, blocks, f = f32_fixc(M, K, sw, out32 and kind == "act")
    if not ok:
        return Launch("generic", blocks, 1, _trips(n4, blocks, 1), False)
    u = min(sw["fixc"], 3 if kind == "apply" else 2)
    untrimmed = ew_blocks((n4 + 1) // 2 if sw["fat"] and sw["fixc"] >= 2 else n4, sw)
    return Launch("fixc%d" % u, blocks, u, _trips(n4, blocks, u), blocks != untrimmed)


def sums_launch(M, K, sw):
    ok, blocks, _ = f32_fixc(M, K, sw)
    return "sums_taken" if ok else "sums_declined"


def sums_lds_bytes(K):
    """Dynamic LDS of a taken column-sums pass: below 256 channel quads the parameters go through a table of 6 floats a channel."""
    return 24 * K if K // 4 < 256 else 0


def reduce_geometry(M, K, bf16):
    K4 = K // 4
    slab = min(K4, 8)
    slabs = -(-K4 // slab)
    groups = 256 // slab
    want = min(64, max(1, NUM_CU * 4 // slabs))
    rows_per_block = max(groups * 4, -(-M // want))
    last_kc = K4 - (slabs - 1) * slab
    return dict(slab=slab, slabs=slabs, groups=groups, rows_per_block=rows_per_block, grid_x=-(-M // rows_per_block),
                last_kc=last_kc, ragged=last_kc != slab, kc_divides=256 % last_kc == 0, RT=8 if bf16 else 4)


def pool_bwd_form(H, W, K, sw):
    return "pool_tiled" if sw["tiled"] and (K // 4) % PB_CQ == 0 else "generic"


def channel_class(K):
    K4 = K // 4
    if 256 % K4 == 0:
        return "divides256"
    if K4 % 256 == 0:
        return "f%d" % (K4 // 256)
    return "neither"


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
K_VALUES = (4, 8, 12, 20, 28, 32, 64, 96, 256, 1024, 1536, 2048, 4096)
# beyond the issue's list: K / 4 = 9 and 11 are the smallest with a RAGGED last slab of the reduce pass (8 + 1 and 8 + 3 quads; the
# second with a width that does not divide 256) -- every K / 4 of the list above is below 8 or a multiple of 8
K_EXTRA = (36, 44)
Case = collections.namedtuple("Case", "name M K")
PoolCase = collections.namedtuple("PoolCase", "name B H W K")


def _m_values(K):
    """The smallest row counts at which every branch of the passes exists for this K."""
    g = reduce_geometry(1, K, False)
    ms = {1, 2, 3}
    lo = (4096 * 4 - 1) // K                      # the largest M with n4 < 4096 and the smallest with n4 >= 4096
    ms |= {lo, lo + 1}
    if K == 4:
        ms |= {4095, 4096, 4097}
    if (4096 * 4) % K == 0:
        ms.add(4096 * 4 // K)                     # n4 == 4096, M a power of two where K is
    if (4097 * 4) % K == 0:
        ms.add(4097 * 4 // K)
    if (4095 * 4) % K == 0:
        ms.add(4095 * 4 // K)
    rpb = g["groups"] * 4                        # rows_per_block's floor: one block up to here, two from rpb + 1
    ms |= {rpb - 1, rpb, rpb + 1}
    for rt in (4, 8):
        ms.add(rt * g["groups"] * 2 - 1)          # one below a multiple of RT * groups
    p = 1
    while p * K // 4 < 4096:
        p *= 2
    ms |= {p, 2 * p}                              # powers of two above the threshold: the train-mode apply with real sums
    if K >= 2048:
        f = K // 1024
        ms |= {lo + 1 + i for i in range(1, 2 * f + 1)}       # block counts that are no multiple of f before the trim
    return sorted(m for m in ms if m >= 1 and m * K <= 1 << 20)


# thread trips: with DPFT_EW_BLOCKS_PER_CU=1 the grid is capped at 256 workgroups = 65 536 threads, so a few hundred thousand
# quads make a thread run 1, 2 and 3 trips with a ragged last one (the default cap of 2048 workgroups needs millions)
TRIP_CASES = (("trips-k64-a", 4099, 64), ("trips-k64-b", 8192 + 7, 64), ("trips-k64-c", 16384 + 8192 + 5, 64),
              ("trips-k64-p2", 16384, 64), ("trips-k12", 43691 + 2, 12), ("trips-k96", 5461 + 3, 96),
              ("trips-k1024", 1024 + 3, 1024), ("trips-k2048", 512 + 37, 2048), ("trips-k1536", 341 + 2, 1536),
              # K / 8 = 3 * 256: a capped grid of 256 workgroups is no multiple of 3 (uncapped ones always are: M * 3)
              ("trips-k6144", 90, 6144),
              # a power of two (the train-mode apply carries real sums: Q (y - mu) with Q != 0 beyond the second trip), and the
              # sizes at which the bf16 forms (two quads / octets per thread and trip) make a third, ragged trip
              ("trips-k64-p2b", 32768, 64), ("trips-k12-c", 87400, 12), ("trips-k64-d", 32800, 64))


def build_lattice():
    cases = []
    for K in K_VALUES + K_EXTRA:
        for M in _m_values(K):
            cases.append(Case("m%d-k%d" % (M, K), M, K))
    cases += [Case(*t) for t in TRIP_CASES]
    return cases


def build_pool_lattice():
    cases = []
    for H, W in ((1, 1), (1, 2), (2, 1), (2, 3), (3, 2), (3, 3), (7, 15), (8, 16), (9, 17), (8, 17), (9, 16), (16, 32), (17, 33)):
        for B, K in ((1, 4), (2, 32), (1, 36), (2, 64)):
            if (H, W) in ((16, 32), (17, 33)) and K in (4, 36):
                continue
            cases.append(PoolCase("pool-%dx%d-b%d-k%d" % (H, W, B, K), B, H, W, K))
    return cases


LATTICE = build_lattice()
POOL_LATTICE = build_pool_lattice()
# column sums (dpft_bn_act_sums_f32): K4 < 256 (parameters through the LDS table) and K4 >= 256, taken and declined
SUMS_CASES = (Case("sums-k64", 256, 64), Case("sums-k64-odd", 259, 64), Case("sums-k32", 515, 32), Case("sums-k1024", 16, 1024),
              Case("sums-k1024-b", 19, 1024), Case("sums-k2048", 9, 2048), Case("sums-k96-declined", 200, 96),
              Case("sums-small-declined", 63, 64), Case("sums-k1536-declined", 16, 1536))


def by_name(name):
    for c in LATTICE + POOL_LATTICE + list(SUMS_CASES):
        if c.name == name:
            return c
    raise KeyError(name)


def case_tags(c, sw=None):
    """What a case covers, as (pass, tag) pairs: the dispatch classes of test_bn_lattice.py's coverage count."""
    sw = sw or DEFAULT_SWITCHES
    tags = set()
    n4 = c.M * c.K // 4
    for kind in ("act", "apply"):
        for bf16 in (False, True):
            L = elementwise_launch(kind, c.M, c.K, bf16, sw)
            st = "bf16" if bf16 else "f32"
            tags.add((kind, st + ":" + L.form))
            tags.add((kind, st + ":" + L.form + ":" + channel_class(c.K)))
            tags.add((kind, st + ":trips%d" % min(L.trips, 3)))
            if L.trimmed:
                tags.add((kind, st + ":trimmed"))
    tags.add(("n4", "odd" if n4 % 2 else "even"))
    for t in (4095, 4096, 4097):
        if n4 == t:
            tags.add(("n4", str(t)))
    tags.add(("n4", "below4096" if n4 < 4096 else "from4096"))
    g = reduce_geometry(c.M, c.K, False)
    tags.add(("reduce", "K4<8" if c.K // 4 < 8 else "K4>=8"))
    if g["ragged"]:
        tags.add(("reduce", "ragged-last-slab"))
    if not g["kc_divides"]:
        tags.add(("reduce", "kc-not-dividing-256"))
    if c.M % g["rows_per_block"]:
        tags.add(("reduce", "M-off-rows_per_block"))
    if g["grid_x"] > 1:
        tags.add(("reduce", "several-row-blocks"))
    if c.M == 1:
        tags.add(("reduce", "M=1"))
    if c.M in (g["groups"] * 4 - 1, g["groups"] * 4 + 1):
        tags.add(("reduce", "rows_per_block+-1"))
    for rt in (4, 8):
        if (c.M + 1) % (rt * g["groups"]) == 0:
            tags.add(("reduce", "one-below-RT%d-groups" % rt))
    tags.add(("K", "K%8!=0" if c.K % 8 else "K%8==0"))
    return tags


REQUIRED_TAGS = {
    ("act", "f32:generic"), ("act", "f32:fixc2"), ("act", "bf16:generic"), ("act", "bf16:wide16"), ("act", "bf16:wide16_fixc"),
    ("apply", "f32:generic"), ("apply", "f32:fixc2"), ("apply", "bf16:generic"), ("apply", "bf16:wide16"), ("apply", "bf16:wide16_fixc"),
    ("act", "f32:fixc2:divides256"), ("act", "f32:fixc2:f2"), ("act", "f32:fixc2:f4"), ("act", "f32:generic:neither"),
    ("act", "bf16:wide16_fixc:divides256"), ("act", "bf16:wide16_fixc:f2"), ("act", "bf16:wide16:neither"),
    ("act", "f32:trimmed"), ("apply", "f32:trimmed"),
    ("act", "f32:trips2"), ("apply", "f32:trips2"),
    ("n4", "odd"), ("n4", "4095"), ("n4", "4096"), ("n4", "4097"), ("n4", "below4096"), ("n4", "from4096"),
    ("reduce", "K4<8"), ("reduce", "ragged-last-slab"), ("reduce", "kc-not-dividing-256"), ("reduce", "M-off-rows_per_block"),
    ("reduce", "several-row-blocks"), ("reduce", "M=1"), ("reduce", "rows_per_block+-1"), ("reduce", "one-below-RT4-groups"),
    ("reduce", "one-below-RT8-groups"), ("K", "K%8!=0"), ("K", "K%8==0"),
}
# what only a changed switch reaches
REQUIRED_TAGS_BY_SWITCH = {
    "per_cu=1": {("act", "f32:trips2"), ("act", "f32:trips3"), ("apply", "f32:trips3"), ("act", "bf16:trips2"), ("apply", "bf16:trips2"),
                 ("act", "bf16:trips3"), ("apply", "bf16:trips3"), ("act", "bf16:trimmed"), ("apply", "bf16:trimmed")},
    "fixc=0": {("act", "f32:generic:divides256"), ("act", "bf16:wide16:divides256")},
    "fixc=1": {("act", "f32:fixc1"), ("apply", "f32:fixc1")},
    "fixc=3": {("apply", "f32:fixc3"), ("act", "f32:fixc2")},
    "wide16=0": {("act", "bf16:generic:divides256"), ("apply", "bf16:generic:f2")},
    "fat=0": {("act", "f32:fixc2"), ("apply", "f32:fixc2:f4")},
}


# ---------------------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------------------
def _gen(name):
    g = torch.Generator()
    g.manual_seed(int.from_bytes(name.encode()[-8:].rjust(8, b"\0"), "little") % (2 ** 31) + len(name))
    return g


def _pick(g, values, n):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), (n,), generator=g)]


def _ints(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def exact_block(g, K):
    """A BN block (4, K) fp64: mean, scale = gamma * invstd, beta, invstd; and gamma."""
    mean = _ints(g, -1, 1, (K,))
    invstd = _pick(g, (0.5, 1.0, 2.0), K)
    gamma = _pick(g, (0.5, 1.0, -1.0, -0.5), K)
    beta = _pick(g, (-1.0, -0.5, 0.0, 0.5, 1.0), K)
    return torch.stack([mean, gamma * invstd, beta, invstd]), gamma


def exact_operands(c):
    """fp64 tensors of the exact tier for an (M, K) case."""
    g = _gen(c.name)
    M, K = c.M, c.K
    o = dict(y=_ints(g, -3, 3, (M, K)), res=_ints(g, -3, 3, (M, K)), dout=_ints(g, -2, 2, (M, K)))
    o["bnp"], o["gamma"] = exact_block(g, K)
    o["rbnp"], _ = exact_block(g, K)
    a0, a1 = _pick(g, (0.0, 0.5, -0.5, 1.0, -1.0), K), _pick(g, (0.0, 0.5, -0.5), K)
    o["a"] = torch.stack([a0, a1])
    o["sums_in"] = o["a"] * M                     # what the train-mode apply is fed, where exact (apply_sums_exact)
    return o


def apply_sums_exact(M):
    """May the train-mode apply of the exact tier carry sums = M * a?  The kernels multiply by fl(1 / M): the products are a again
    -- also inside a fused multiply-add, which keeps them unrounded -- only if fl(1 / M) is exact."""
    inv = np.float32(1.0) / np.float32(M)
    return float(inv) * M == 1.0


def float_operands(c, seed=0):
    """Gaussian data: channel e has |mean| / std = (1, 30, 1000)[e % 3], invstd log-uniform in [1e-3, 1e3]."""
    g = _gen(c.name + "/float%d" % seed)
    M, K = c.M, c.K
    ratio = torch.tensor([1.0, 30.0, 1000.0], dtype=torch.float64)[torch.arange(K) % 3]
    invstd = 10.0 ** (torch.rand(K, generator=g, dtype=torch.float64) * 6 - 3)
    sign = torch.where(torch.rand(K, generator=g) < 0.5, -1.0, 1.0).double()
    mean = sign * ratio / invstd
    gamma = torch.randn(K, generator=g, dtype=torch.float64) * 0.5 + 1.0
    beta = torch.randn(K, generator=g, dtype=torch.float64)
    f32 = lambda t: t.float().double()
    o = dict(y=f32(mean + torch.randn(M, K, generator=g, dtype=torch.float64) / invstd),
             res=f32(torch.randn(M, K, generator=g, dtype=torch.float64)), dout=f32(torch.randn(M, K, generator=g, dtype=torch.float64)))
    o["bnp"] = f32(torch.stack([f32(mean), f32(gamma) * f32(invstd), beta, f32(invstd)]))
    o["gamma"] = f32(gamma)
    rmean, ristd = torch.randn(K, generator=g, dtype=torch.float64), 10.0 ** (torch.rand(K, generator=g, dtype=torch.float64) - 0.5)
    o["rbnp"] = f32(torch.stack([rmean, f32(gamma.flip(0)) * f32(ristd), beta.flip(0), ristd]))
    return o


def to_storage(t, bf16):
    """fp64 -> the storage type's values, as fp64 (what the kernel reads)."""
    return (t.bfloat16() if bf16 else t.float()).double()


# ---------------------------------------------------------------------------------------------------------------------------------
# the fp64 reference
# ---------------------------------------------------------------------------------------------------------------------------------
def bn(v, bnp):
    return (v - bnp[0]) * bnp[1] + bnp[2]


def mask_bytes(v):
    """(M, K) -> (M, K / 4) uint8: bit e of a byte = element e of its four channels is > 0."""
    b = (v > 0).reshape(v.shape[0], -1, 4).to(torch.int64)
    return (b * torch.tensor([1, 2, 4, 8])).sum(-1).to(torch.uint8)


def mask_from_bytes(m8):
    return ((m8.to(torch.int64)[..., None] >> torch.arange(4)) & 1).reshape(m8.shape[0], -1).bool()


def ref_act(y, bnp, res=None, rbnp=None, relu=True):
    v = bn(y, bnp)
    if res is not None:
        v = v + (bn(res, rbnp) if rbnp is not None else res)
    if relu:
        v = v.clamp_min(0.0)
    return v


def ref_mask(kind, y, mask8=None, out=None, mbnp=None):
    if kind == "mask8":
        return mask_from_bytes(mask8)
    if kind == "out":
        return out > 0
    if kind == "mask_bnp":
        return bn(y, mbnp) > 0
    return torch.ones_like(y, dtype=torch.bool)


def ref_reduce(y, dout, bnp, mask):
    dz = torch.where(mask, dout, torch.zeros_like(dout))
    xhat = (y - bnp[0]) * bnp[3]
    return torch.stack([dz.sum(0), (dz * xhat).sum(0)])


def ref_apply(y, dout, bnp, gamma, sums, mask, frozen):
    M = y.shape[0]
    dz = torch.where(mask, dout, torch.zeros_like(dout))
    xhat = (y - bnp[0]) * bnp[3]
    if frozen:
        return gamma * bnp[3] * dz
    return gamma * bnp[3] * (dz - sums[0] / M - xhat * sums[1] / M)


def apply_terms(y, dout, bnp, gamma, sums, mask, frozen):
    """Sum of the magnitudes of the terms of the defining expression (the float tier's T)."""
    M = y.shape[0]
    dz = torch.where(mask, dout, torch.zeros_like(dout)).abs()
    xhat = ((y - bnp[0]) * bnp[3]).abs()
    a = (gamma * bnp[3]).abs()
    if frozen:
        return a * dz
    return a * (dz + sums[0].abs() / M + xhat * sums[1].abs() / M)


def act_terms(y, bnp, res=None, rbnp=None):
    t = ((y - bnp[0]) * bnp[1]).abs() + bnp[2].abs()
    if res is not None:
        t = t + (((res - rbnp[0]) * rbnp[1]).abs() + rbnp[2].abs() if rbnp is not None else res.abs())
    return t


def float_bound(terms, ref, bf16, c=C_BOUND):
    b = c * U32 * terms
    if not bf16:
        return b
    half_ulp = U16 * 2.0 ** torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))      # of an 8-bit significand
    return b + half_ulp


# max-pool 3 x 3 / stride 2 / pad 1 of a = relu(bn(y)), NHWC.  Tie rule (what both backward kernels implement): a window's
# gradient goes to its FIRST maximum in scan order (rows, then columns, of the window's valid pixels; strict > moves on), and to
# nobody if that maximum is 0 (relu did not pass).
def pool_size(n):
    return (n - 1) // 2 + 1


def ref_pool(y, bnp, last_max=False):
    """-> (out (B, PH, PW, K), arg (B, PH, PW, K) index di * 3 + dj of the chosen pixel)."""
    a = bn(y, bnp).clamp_min(0.0)
    B, H, W, K = a.shape
    PH, PW = pool_size(H), pool_size(W)
    out = torch.full((B, PH, PW, K), -1.0, dtype=torch.float64)
    arg = torch.full((B, PH, PW, K), -1, dtype=torch.int64)
    for ph in range(PH):
        for pw in range(PW):
            for di in range(3):
                for dj in range(3):
                    h, w = 2 * ph - 1 + di, 2 * pw - 1 + dj
                    if not (0 <= h < H and 0 <= w < W):
                        continue
                    v = a[:, h, w]
                    better = (v >= out[:, ph, pw]) if last_max else (v > out[:, ph, pw])
                    out[:, ph, pw] = torch.where(better, v, out[:, ph, pw])
                    arg[:, ph, pw] = torch.where(better, torch.full_like(arg[:, ph, pw], di * 3 + dj), arg[:, ph, pw])
    return out, arg


def ref_pool_bwd(y, bnp, dout):
    a = bn(y, bnp).clamp_min(0.0)
    B, H, W, K = a.shape
    _, arg = ref_pool(y, bnp)
    dz = torch.zeros_like(a)
    for ph in range(arg.shape[1]):
        for pw in range(arg.shape[2]):
            for di in range(3):
                for dj in range(3):
                    h, w = 2 * ph - 1 + di, 2 * pw - 1 + dj
                    if 0 <= h < H and 0 <= w < W:
                        dz[:, h, w] += torch.where(arg[:, ph, pw] == di * 3 + dj, dout[:, ph, pw], torch.zeros_like(dout[:, ph, pw]))
    return torch.where(a > 0, dz, torch.zeros_like(dz))


def pool_operands(c):
    """Few distinct values on purpose: most windows hold ties, many hold nothing above zero."""
    g = _gen(c.name)
    o = dict(y=_ints(g, -2, 2, (c.B, c.H, c.W, c.K)), dout=_ints(g, -3, 3, (c.B, pool_size(c.H), pool_size(c.W), c.K)))
    o["bnp"], _ = exact_block(g, c.K)
    if c.H * c.W >= 4:
        o["y"][:, : c.H // 2 + 1] = o["y"][:, :1]                 # planted: whole rows equal -> every window there is one tie
    return o


# column sums in the library's fixed-point format (common.h): [4][K] 64-bit words: sum y as (count of fours, units of 2^-46 below
# four), then sum y^2 the same way
def encode_sums(s1, s2):
    words = []
    for s in (s1, s2):
        h = torch.floor(s / 4.0)
        lo = (s - h * 4.0) * 2.0 ** 46
        assert bool((lo == lo.floor()).all()) and bool((lo < 2.0 ** 48).all())
        words += [h.to(torch.int64), lo.to(torch.int64)]
    return torch.stack(words)


def sums_operands(c):
    """Exact tier for dpft_bn_act_sums_f32: integer means, variances in {1/4, 1, 4} and eps = 0, so that the block the kernel
    derives (mean = S1 / M, invstd = 1 / sqrt(S2 / M - mean^2)) is dyadic."""
    o = exact_operands(c)
    g = _gen(c.name + "/sums")
    for side, key in (("y", "bnp"), ("res", "rbnp")):
        mean, invstd = o[key][0], o[key][3]
        var = 1.0 / (invstd * invstd)
        gamma = o[key][1] / invstd
        o[side + "_sums"] = encode_sums(mean * c.M, (var + mean * mean) * c.M)
        o[side + "_gamma"], o[side + "_beta"] = gamma, o[key][2]
    return o


# ---------------------------------------------------------------------------------------------------------------------------------
# exactness proofs: the kernels' expressions replayed in numpy float32
# ---------------------------------------------------------------------------------------------------------------------------------
def _f(t):
    return t.numpy().astype(np.float32)


def _fma(a, b, c):
    """float32 fused multiply-add of float32 arrays (the product of two float32 is exact in float64)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def replay_act(y, bnp, res, rbnp, relu):
    y, res = _f(y), (None if res is None else _f(res))
    mu, sc, be = _f(bnp[0]), _f(bnp[1]), _f(bnp[2])
    v = _fma(y - mu, sc, be)
    if res is not None:
        r = res
        if rbnp is not None:
            r = _fma(res - _f(rbnp[0]), _f(rbnp[1]), _f(rbnp[2]))
        v = v + r
    return np.maximum(v, np.float32(0)) if relu else v


def replay_apply(y, dz, bnp, gamma, sums, M, frozen, form):
    """form: 'generic' (rounded after every operation), 'generic-fused' (products unrounded inside the subtractions), 'fixc'
    (the kernels' A d + (Q (y - mu) + P)) or 'fixc-uncentred' (A d + (Q y + P), see FOUND AND FIXED)."""
    y, d = _f(y), _f(dz)
    mu, is_, ga, s0, s1 = _f(bnp[0]), _f(bnp[3]), _f(gamma), _f(sums[0]), _f(sums[1])
    invM = np.float32(0) if frozen else np.float32(1.0) / np.float32(M)
    if form == "fixc":                    # the fixed-channel kernels: y centred before the multiply
        A = ga * is_
        Q = -A * is_ * (s1 * invM)
        P = -A * (s0 * invM)
        return _fma(A, d, _fma(Q, y - mu, P))
    if form == "fixc-uncentred":          # what the kernels computed before this lattice: Q mu folded into P
        A = ga * is_
        Q = -A * is_ * (s1 * invM)
        P = -A * (s0 * invM) - Q * mu
        return _fma(A, d, _fma(Q, y, P))
    xh = (y - mu) * is_
    if form == "generic":
        return ga * is_ * (d - s0 * invM - xh * s1 * invM)
    t = _fma(-s0, np.full_like(s0, invM), d)
    t = _fma(-(xh * s1), np.full_like(y, invM), t)
    return ga * is_ * t


def replay_reduce_terms(y, dz, bnp):
    y, d = _f(y), _f(dz)
    return d, d * ((y - _f(bnp[0])) * _f(bnp[3]))


ACT_VARIANTS = (dict(res=False, rbn=False, relu=False), dict(res=False, rbn=False, relu=True), dict(res=True, rbn=False, relu=True),
                dict(res=True, rbn=True, relu=True), dict(res=True, rbn=True, relu=False))


def exact_proof(c, o=None):
    """Asserts that the exact tier of case c is exact in float32 for every kernel expression and in bf16 for every stored value.
    -> dict(train_sums=bool): whether the train-mode apply carries non-zero sums (apply_sums_exact)."""
    o = o or exact_operands(c)
    eq = lambda a, b: np.array_equal(a.astype(np.float64), b.numpy())
    bf = lambda t: bool((t.bfloat16().double() == t).all())
    for k in ("y", "res", "dout"):
        assert bf(o[k]), (c.name, k)
    outs = {}
    for v in ACT_VARIANTS:
        res, rbnp = (o["res"] if v["res"] else None), (o["rbnp"] if v["rbn"] else None)
        want = ref_act(o["y"], o["bnp"], res, rbnp, v["relu"])
        assert eq(replay_act(o["y"], o["bnp"], res, rbnp, v["relu"]), want) and bf(want), (c.name, v)
        outs[tuple(v.values())] = want
    out = outs[(True, False, True)]
    masks = dict(none=ref_mask("none", o["y"]), out=out > 0, mask_bnp=bn(o["y"], o["rbnp"]) > 0, mask_self=bn(o["y"], o["bnp"]) > 0,
                 mask8=mask_from_bytes(mask_bytes(out)))
    assert torch.equal(masks["out"], masks["mask8"])
    train_sums = apply_sums_exact(c.M)
    for name, m in masks.items():
        dz = torch.where(m, o["dout"], torch.zeros_like(o["dout"]))
        t0, t1 = replay_reduce_terms(o["y"], dz, o["bnp"])
        xhat = (o["y"] - o["bnp"][0]) * o["bnp"][3]
        assert eq(t0, dz) and eq(t1, dz * xhat), (c.name, name)
        assert float((dz * xhat).abs().sum(0).max()) < 2 ** 23 and float(dz.abs().sum(0).max()) < 2 ** 23      # every partial sum is exact
        sums = ref_reduce(o["y"], o["dout"], o["bnp"], m)
        assert bool((sums.float().double() == sums).all())
        for frozen in (False, True):
            fed = o["sums_in"] if (train_sums or frozen) else torch.zeros_like(o["sums_in"])
            want = ref_apply(o["y"], o["dout"], o["bnp"], o["gamma"], fed, m, frozen)
            for form in ("generic", "generic-fused", "fixc"):
                got = replay_apply(o["y"], dz, o["bnp"], o["gamma"], fed, c.M, frozen, form)
                assert eq(got, want), (c.name, name, frozen, form)
            assert bf(want), (c.name, name, frozen)
    return dict(train_sums=train_sums)


def float_selfcheck(c, bf16=False):
    """The float tier on the CPU: the float32 replay of both apply forms and of act stays within the bound with c halved.
    -> the largest error / bound ratio per form (for the record)."""
    o = float_operands(c)
    st = lambda t: to_storage(t, bf16)
    y, res, dout = st(o["y"]), st(o["res"]), st(o["dout"])
    worst = {}
    for v in ACT_VARIANTS:
        r, rb = (res if v["res"] else None), (o["rbnp"] if v["rbn"] else None)
        want = ref_act(y, o["bnp"], r, rb, v["relu"])
        err = torch.from_numpy(replay_act(y, o["bnp"], r, rb, v["relu"]).astype(np.float64)) - want
        bound = float_bound(act_terms(y, o["bnp"], r, rb), want, False, C_BOUND / 2)
        worst["act"] = max(worst.get("act", 0.0), float((err.abs() / bound).max()))
    mask = ref_act(y, o["bnp"], res, None, True) > 0
    sums = ref_reduce(y, dout, o["bnp"], mask).float().double()
    dz = torch.where(mask, dout, torch.zeros_like(dout))
    for frozen in (False, True):
        want = ref_apply(y, dout, o["bnp"], o["gamma"], sums, mask, frozen)
        bound = float_bound(apply_terms(y, dout, o["bnp"], o["gamma"], sums, mask, frozen), want, False, C_BOUND / 2)
        for form in ("generic", "generic-fused", "fixc", "fixc-uncentred"):
            err = torch.from_numpy(replay_apply(y, dz, o["bnp"], o["gamma"], sums, c.M, frozen, form).astype(np.float64)) - want
            ratio = (err.abs() / bound.clamp_min(1e-300))
            for i, name in enumerate(("r1", "r30", "r1000")):
                key = "%s%s:%s" % (form, ":frozen" if frozen else "", name)
                worst[key] = max(worst.get(key, 0.0), float(ratio[:, i::3].max()))
    return worst


# one float-tier case per dispatch class (default switches)
FLOAT_CASES = (Case("float-generic-k96", 211, 96), Case("float-small-k12", 37, 12), Case("float-fixc-k64", 259, 64),
               Case("float-fixc-k2048", 9, 2048), Case("float-fixc-k32", 515, 32),
               # from 4096 octets: the fixed-channel forms of the 16-byte bf16 kernels
               Case("float-fixc16-k32", 1027, 32), Case("float-fixc16-k4096", 9, 4096))
# c = 8 counts the roundings of the longest chain, so the float32 replay is guaranteed to stay within c, not within c / 2: the
# halved self-check is a statement about eight roundings not lining up.  This case's every-operation-rounded generic replay
# reaches 1.13 of the HALVED bound (left open); it is held to the full bound on the CPU as on the device.
SELFCHECK_FULL_BOUND_ONLY = ("float-fixc16-k4096",)
