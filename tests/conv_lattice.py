"""TEST INFRASTRUCTURE -- the geometry lattice of tests/test_conv_lattice.py (CPU) and tests/test_gpu_conv_geometry.py (GPU).

The convolution library accepts any B, H, W, C, K, kh, kw, stride, pad with positive sizes and dispatches to more than a dozen
kernels; the network's own shapes all have kh == kw, pad == k // 2, stride <= 2 and maps larger than the filter.  A transposed
row/column decode, a wrong border tap, a leftover input row or a ragged channel tile gives the same answer on those.  The lattice
walks the descriptor space instead: non-square filters, pad 0 .. >= filter, stride 1 .. 3 (also above the filter), channel counts
on either side of every vector width, row counts M on either side of every tile height, one-pixel maps, maps smaller than the
filter and input rows no output reaches.

Operands are small integers: x, w, dy, bias in [-8, 8]; BatchNorm blocks with integer mean / shift and a power-of-two scale.
Every product and every partial sum of every summation order is then an integer (or a dyadic fraction) far below 2^24 in
magnitude, exactly representable in fp32, and every operand is exact in bf16 -- so the fp32 MFMA kernels, the 3 x bf16 split
kernels and the bf16-operand kernels must all return the fp64 result BIT FOR BIT.  No tolerance, and one wrong tap cannot hide.

No GPU code here: the case list, the operands, the fp64 reference (F.conv2d + autograd) and a six-loop numpy restatement."""
import itertools
import random
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

FILTERS = [(1, 1), (3, 3), (1, 3), (3, 1), (2, 2), (5, 3), (2, 7), (7, 7), (8, 8)]
STRIDES = [1, 2, 3]
PAD_KINDS = ["0", "1", "2", "half", "over"]                 # "half" = max(kh, kw) // 2, "over" >= max(kh, kw)
C_VALUES = [1, 3, 4, 5, 6, 16, 32, 64, 96, 128, 192]
K_VALUES = [1, 3, 5, 16, 17, 32, 64, 66, 68, 100, 128, 132, 192]
M_TARGETS = [1, 63, 64, 65, 127, 129, 255, 257]             # either side of the 64 / 128 / 256-row tiles
M_KINDS = [str(m) for m in M_TARGETS] + ["thousands"]       # "thousands": 2000 <= M (several row tiles)
EDGES = ["H=1", "W=1", "H<kh", "leftover"]                  # leftover: (H + 2 pad - kh) % stride != 0
CLASSES = ["c64", "c32", "thin", "matcher", "generic"]
VMAX = 8                                                    # |operand| <= 8
ELEMS_MAX = 250_000                                         # B * H * W * C of a sampled case (the named exceptions are larger)

Case = namedtuple("Case", "name B H W C K kh kw stride pad cls")


def out_size(c):
    return (c.H + 2 * c.pad - c.kh) // c.stride + 1, (c.W + 2 * c.pad - c.kw) // c.stride + 1


def rows(c):
    oh, ow = out_size(c)
    return c.B * oh * ow


def is_conv16(c):
    return c.C == 16 and c.K == 16 and (c.kh, c.kw, c.stride, c.pad) == (3, 3, 1, 1)


def is_thin1x1(c):
    return (c.kh, c.kw, c.stride, c.pad) == (1, 1, 1, 0) and ((c.K == 16 and c.C in (3, 6)) or (c.K == 3 and c.C == 6))


def is_stem7(c):
    return (c.kh, c.kw, c.stride, c.pad, c.C, c.K) == (7, 7, 2, 3, 3, 64) and rows(c) >= 131072


def dispatch_class(B, H, W, C, K, kh, kw, stride, pad):
    c = Case("", B, H, W, C, K, kh, kw, stride, pad, "")
    if is_conv16(c) or is_thin1x1(c) or is_stem7(c):
        return "matcher"
    if C % 64 == 0:
        return "c64"
    if C % 32 == 0 and K % 4 == 0:
        return "c32"
    if C <= 4:
        return "thin"
    return "generic"


def class_axes(cls):
    """The axis values a dispatch class admits (the matchers pin their own geometry: no axes)."""
    if cls == "matcher":
        return {}
    Cs = {"c64": [64, 128, 192], "c32": [32, 96], "thin": [1, 3, 4], "generic": [5, 6, 16, 32, 96]}[cls]
    Ks = [k for k in K_VALUES if k % 4 == 0] if cls == "c32" else list(K_VALUES)
    return {"filter": list(FILTERS), "stride": list(STRIDES), "pad": list(PAD_KINDS), "C": Cs, "K": Ks, "M": list(M_KINDS),
            "edge": list(EDGES)}


def case_tags(c):
    """(axis, value) pairs a case covers."""
    oh, ow = out_size(c)
    m = c.B * oh * ow
    tags = {("filter", (c.kh, c.kw)), ("stride", c.stride), ("C", c.C), ("K", c.K)}
    kmax = max(c.kh, c.kw)
    if c.pad <= 2:
        tags.add(("pad", str(c.pad)))
    if c.pad == kmax // 2:
        tags.add(("pad", "half"))
    if c.pad >= kmax:
        tags.add(("pad", "over"))
    if m in M_TARGETS:
        tags.add(("M", str(m)))
    if m >= 2000:
        tags.add(("M", "thousands"))
    if c.H == 1:
        tags.add(("edge", "H=1"))
    if c.W == 1:
        tags.add(("edge", "W=1"))
    if c.H < c.kh:
        tags.add(("edge", "H<kh"))
    if (c.H + 2 * c.pad - c.kh) % c.stride != 0:
        tags.add(("edge", "leftover"))
    return tags


def make_case(name, B, H, W, C, K, kh, kw, stride, pad):
    c = Case(name, B, H, W, C, K, kh, kw, stride, pad, dispatch_class(B, H, W, C, K, kh, kw, stride, pad))
    oh, ow = out_size(c)
    assert min(B, H, W, C, K, kh, kw, stride) >= 1 and pad >= 0 and oh >= 1 and ow >= 1, c
    check_exactness(c)
    return c


# ---------------------------------------------------------------------------------------------------------------------
# exactness
# ---------------------------------------------------------------------------------------------------------------------
PRO_MAX = 2 * (VMAX + 2) + 2      # |(x - mean) * scale + shift| with |mean|, |shift| <= 2 and scale in {1/2, 1, 2}


def check_exactness(c):
    """Every product and partial sum stays an exactly representable fp32 value, whatever the summation order."""
    taps_c = c.kh * c.kw * c.C
    m = rows(c)
    assert taps_c * VMAX * VMAX < 2 ** 24, c                # forward / data gradient reductions
    assert m * VMAX * VMAX < 2 ** 24, c                     # weight gradient / bias gradient reductions
    assert c.kh * c.kw * c.K * VMAX * VMAX + VMAX < 2 ** 24, c      # data gradient over K (+ the accumulation base)
    # with the BatchNorm + ReLU operand prologue (run where C % 64 == 0) the operand is a multiple of 1/2 up to PRO_MAX: sums
    # are multiples of 1/2
    assert c.C % 64 or (2 * taps_c * PRO_MAX * VMAX < 2 ** 24 and 2 * m * PRO_MAX * VMAX < 2 ** 24), c
    # the inference epilogue: (conv - mean) * scale + shift (+ residual), scale in {1/2, 1, 2}
    assert 2 * (2 * (taps_c * VMAX * VMAX + VMAX) + 2 * VMAX) < 2 ** 24, c
    return True


def bf16_exact(t):
    return bool(torch.equal(t.float().bfloat16().float(), t.float()))


# ---------------------------------------------------------------------------------------------------------------------
# the case list
# ---------------------------------------------------------------------------------------------------------------------
def _pad_of(kind, kh, kw, rng):
    kmax = max(kh, kw)
    return {"0": 0, "1": 1, "2": 2, "half": kmax // 2}[kind] if kind != "over" else kmax + rng.randrange(2)


def _candidate(cls, rng):
    ax = class_axes(cls)
    kh, kw = rng.choice(ax["filter"])
    s = rng.choice(ax["stride"])
    pad = _pad_of(rng.choice(ax["pad"]), kh, kw, rng)
    C, K = rng.choice(ax["C"]), rng.choice(ax["K"])
    mk = rng.choice(ax["M"])
    if mk == "thousands":
        B, oh, ow = rng.choice([1, 2]), rng.randrange(24, 50), rng.randrange(24, 50)
        if B * oh * ow < 2000:
            return None
    else:
        m = int(mk)
        facts = [(b, h, m // (b * h)) for b in (1, 2, 3, 4) if m % b == 0 for h in range(1, m // b + 1) if (m // b) % h == 0]
        B, oh, ow = rng.choice(facts)
    H = (oh - 1) * s + kh - 2 * pad + rng.randrange(s)
    W = (ow - 1) * s + kw - 2 * pad + rng.randrange(s)
    if H < 1 or W < 1 or B * H * W * C > ELEMS_MAX:
        return None
    if dispatch_class(B, H, W, C, K, kh, kw, s, pad) != cls:
        return None
    return (B, H, W, C, K, kh, kw, s, pad)


def _covering_sample(cls, seed, extra):
    """Greedy cover of the class's (axis, value) pairs from seeded random candidates, then ``extra`` more cases that each add
    a (filter, stride) or (C, K) pair not seen yet."""
    rng = random.Random(seed)
    want = {(a, v) for a, vs in class_axes(cls).items() for v in vs}
    got, out, pairs = set(), [], set()
    for _ in range(400):
        if not (want - got) and extra <= 0:
            break
        best, best_gain = None, 0
        for _ in range(300):
            t = _candidate(cls, rng)
            if t is None:
                continue
            c = Case("", *t, cls)
            tags = case_tags(c)
            pp = {("fs", c.kh, c.kw, c.stride), ("ck", c.C, c.K)}
            gain = 4 * len((tags & want) - got) + len(pp - pairs)
            if gain > best_gain:
                best, best_gain = c, gain
        if best is None:
            break
        if not (want - got):
            extra -= 1
        got |= case_tags(best) & want
        pairs |= {("fs", best.kh, best.kw, best.stride), ("ck", best.C, best.K)}
        out.append(best)
    assert not (want - got), (cls, sorted(map(str, want - got)))
    return [make_case(f"{cls}-{i:02d}", *c[1:10]) for i, c in enumerate(out)]


# name, B, H, W, C, K, kh, kw, stride, pad -- the corners the issue names, by hand
CORNERS = [
    # rows and columns of the filter: non-square filters, non-square maps, one pad for both axes
    ("rc-1x3-c64", 2, 5, 9, 64, 64, 1, 3, 1, 1),
    ("rc-3x1-c64", 2, 5, 9, 64, 64, 3, 1, 1, 1),
    ("rc-5x3-c64-s2", 1, 11, 8, 64, 128, 5, 3, 2, 1),
    ("rc-2x7-c128", 1, 6, 13, 128, 64, 2, 7, 1, 3),
    ("rc-2x7-c128-s2", 2, 9, 16, 128, 64, 2, 7, 2, 2),
    ("rc-5x3-generic", 2, 9, 7, 6, 17, 5, 3, 1, 2),
    ("rc-2x7-thin-s3", 2, 8, 20, 3, 16, 2, 7, 3, 1),
    ("rc-3x1-c32", 1, 9, 6, 32, 68, 3, 1, 2, 0),
    # pad != k // 2
    ("pad0-3x3-c64", 2, 8, 10, 64, 64, 3, 3, 1, 0),
    ("pad0-3x3-generic", 2, 8, 10, 6, 16, 3, 3, 1, 0),
    ("pad3-3x3-c64", 1, 4, 5, 64, 64, 3, 3, 1, 3),             # pad = filter: the outer ring of outputs sees padding only
    ("pad4-3x3-c64-s2", 2, 5, 6, 64, 128, 3, 3, 2, 4),
    ("pad4-3x3-c32-s2", 2, 5, 6, 96, 68, 3, 3, 2, 4),
    ("pad2-1x1-c64", 2, 3, 4, 64, 64, 1, 1, 1, 2),             # 1x1 with padding: not the streaming / thin 1x1 forms
    ("leftover-3x3-c64-s2", 2, 10, 12, 64, 64, 3, 3, 2, 1),    # (10 + 2 - 3) % 2 = 1
    ("leftover-1x1-c128-s2", 2, 8, 10, 128, 64, 1, 1, 2, 0),   # three of four parity classes empty, last row / column unreached
    ("leftover-2x2-c64-s3", 2, 10, 9, 64, 64, 2, 2, 3, 0),     # stride above the filter: rows 2, 5, 8 (and 9) unreached
    # stride 3 on the C % 64 == 0 path, stride above the filter
    ("s3-3x3-c64", 2, 9, 11, 64, 64, 3, 3, 3, 1),
    ("s3-1x1-c64", 2, 7, 8, 64, 64, 1, 1, 3, 0),
    ("s3-tiny-c64", 2, 2, 2, 64, 64, 3, 3, 3, 1),              # parity classes with ph >= H
    ("s3-H1-c64-1x1-p1", 1, 1, 7, 64, 64, 1, 1, 3, 1),         # no tap reaches the only input row: dx = 0
    ("s3-2x7-generic", 1, 7, 19, 16, 5, 2, 7, 3, 2),
    # parity-class data gradients with a workspace: enough rows per class to fill the chip (larger than ELEMS_MAX)
    ("classes-s2-3x3-c192", 2, 74, 75, 192, 64, 3, 3, 2, 1),
    ("classes-s3-2x2-c192", 2, 111, 110, 192, 64, 2, 2, 3, 0),
    ("classes-s3-5x3-c192", 2, 110, 112, 192, 128, 5, 3, 3, 2),
    ("classes-s2-1x1-c192", 2, 74, 76, 192, 64, 1, 1, 2, 0),
    # ragged channel counts
    ("c96-k64-3x3", 2, 6, 7, 96, 64, 3, 3, 1, 1),              # C % 64 == 32: vector weight gradient, ctiles = cdiv(C, 64)
    ("c32-k132-1x1", 2, 6, 7, 32, 132, 1, 1, 1, 0),
    ("c160-like-c96-k192", 1, 9, 9, 96, 192, 3, 3, 2, 1),
    ("c64-k1", 2, 8, 8, 64, 1, 3, 3, 1, 1),                    # K % 4 != 0 on the vector forward: N = 1, 3, 5, 66
    ("c64-k3", 2, 8, 8, 64, 3, 3, 3, 1, 1),
    ("c128-k5", 2, 8, 8, 128, 5, 1, 1, 1, 0),
    ("c64-k66", 2, 8, 8, 64, 66, 3, 3, 1, 1),
    ("c192-k66-splitk", 1, 4, 4, 192, 66, 7, 7, 1, 3),         # deep reduction, few tiles: a K split with N % 4 != 0
    ("c192-k3-splitk", 1, 4, 4, 192, 3, 8, 8, 1, 4),
    ("c64-k68", 2, 8, 8, 64, 68, 3, 3, 1, 1),                  # K % 64 in {4, 36}
    ("c64-k100", 2, 8, 8, 64, 100, 3, 3, 1, 1),
    ("c128-k132", 2, 8, 8, 128, 132, 1, 1, 1, 0),
    ("c1-k16", 2, 9, 8, 1, 16, 3, 3, 1, 1),                    # either side of the thin data gradient's C <= 4
    ("c4-k16-s2", 2, 9, 8, 4, 16, 3, 3, 2, 1),
    ("c4-k17", 2, 9, 8, 4, 17, 3, 3, 1, 1),                    # thin channels, K % 4 != 0: generic data gradient
    ("c5-k16", 2, 9, 8, 5, 16, 3, 3, 1, 1),
    # maps smaller than a tile or than the filter
    ("H1-c64", 2, 1, 9, 64, 64, 3, 3, 1, 1),
    ("W1-c64", 2, 9, 1, 64, 64, 3, 3, 1, 1),
    ("H1W1-c64-7x7", 1, 1, 1, 64, 64, 7, 7, 1, 3),             # M = 1
    ("H1W1-generic-8x8", 1, 1, 1, 6, 5, 8, 8, 2, 4),
    ("Hltk-c128-8x8", 1, 3, 5, 128, 64, 8, 8, 1, 4),
    ("Hltk-thin-5x3", 2, 2, 9, 3, 32, 5, 3, 2, 2),
    ("M63-c64", 1, 7, 9, 64, 64, 3, 3, 1, 1),
    ("M65-c64", 1, 5, 13, 64, 128, 3, 3, 1, 1),
    ("M127-c64", 1, 1, 127, 64, 64, 1, 3, 1, 1),
    ("M129-c64", 1, 3, 43, 64, 64, 3, 3, 1, 1),
    ("M255-c64", 1, 15, 17, 64, 192, 3, 3, 1, 1),
    ("M257-c64", 1, 257, 1, 64, 64, 3, 1, 1, 1),
    # the matchers
    ("conv16", 2, 19, 23, 16, 16, 3, 3, 1, 1),
    ("conv16-H1", 1, 1, 5, 16, 16, 3, 3, 1, 1),
    ("conv16-M257", 1, 257, 1, 16, 16, 3, 3, 1, 1),
    ("thin1x1-c3", 2, 19, 23, 3, 16, 1, 1, 1, 0),
    ("thin1x1-c6-M1", 1, 1, 1, 6, 16, 1, 1, 1, 0),
    ("thin1x1-c6-k3", 2, 21, 17, 6, 3, 1, 1, 1, 0),
    ("stem7", 2, 362, 726, 3, 64, 7, 7, 2, 3),                 # >= 131072 output pixels (LDS-tiled weight gradient), leftover row
]
# >= 2 GFLOP with a non-square filter: the automatic 3 x bf16 split (forward, stride-1 data gradient; weight gradient where
# K, C >= 128)
BIG = [
    ("x3-5x3-c64", 2, 96, 92, 64, 64, 5, 3, 1, 1),
    ("x3-2x7-c128", 2, 48, 56, 128, 128, 2, 7, 1, 2),
]
LARGE_NAMES = {"stem7", "x3-5x3-c64", "x3-2x7-c128", "classes-s2-3x3-c192", "classes-s3-2x2-c192", "classes-s3-5x3-c192",
               "classes-s2-1x1-c192"}
SAMPLE_EXTRA = {"c64": 8, "c32": 3, "thin": 3, "generic": 5}


def build_lattice():
    cases = [make_case(*t) for t in CORNERS + BIG]
    for i, cls in enumerate(("c64", "c32", "thin", "generic")):
        cases += _covering_sample(cls, 20261017 + i, SAMPLE_EXTRA[cls])
    seen = set()
    for c in cases:
        assert c.name not in seen, c.name
        seen.add(c.name)
    return cases


LATTICE = build_lattice()
# the compute modes (ops.conv_set_compute name, split switch), the forced tiles and the case lists they run on -- shared by the
# host test of the launch plan (tests/test_conv_lattice.py) and the GPU tests (tests/test_gpu_conv_geometry.py)
MODES = {"fp32": ("fp32", False), "fp32+split": ("fp32", True), "bf16x3": ("bf16x3", True), "bf16": ("bf16", True)}
FORCE_TILES = ["128,128,1", "128,64,2", "64,128,1", "64,64,3"]
FORCE_WGRADS = ["128,1", "128,3", "64,1", "64,5"]
BNACT = "dpft_conv2d_nhwc_fwd_bnact_f32"
WGRAD_PRO = "dpft_conv2d_nhwc_wgrad_f32 + prologue"


# (of the large cases one goes through the forced tiles: a strided data gradient that takes the parity classes WITH a workspace)
C64 = [c for c in LATTICE if c.cls == "c64" and (c.name not in LARGE_NAMES or c.name == "classes-s3-2x2-c192")]
WVEC = [c for c in LATTICE if c.C % 32 == 0 and c.K % 4 == 0 and c.name not in LARGE_NAMES]


def refusal(c, entry):
    """Message fragment of the DPFT_ERR_ARG with which ``entry`` refuses this geometry, or None where it computes it.  Two
    refusals, both for K % 4 != 0: the inference epilogue takes the output channels four at a time, and the weight gradient's
    operand prologue exists in the vector kernels only (C % 32 == 0 and K % 4 == 0).  Every other entry computes every case.
    Each refusal is asserted through the C-ABI without a GPU (tests/test_conv_lattice.py, tests/test_host.py)."""
    if entry == BNACT and c.K % 4:
        return "conv fwd_bnact: K % 4 == 0 needed"
    if entry == WGRAD_PRO and (c.C % 32 or c.K % 4):
        return "conv wgrad: fused prologue needs C % 32 == 0 and K % 4 == 0"
    return None


def by_name(name):
    return next(c for c in LATTICE if c.name == name)


# ---------------------------------------------------------------------------------------------------------------------
# operands and the fp64 reference
# ---------------------------------------------------------------------------------------------------------------------
def _seed(c):
    return 7919 * (c.B + 3 * c.H + 5 * c.W + 7 * c.C + 11 * c.K + 13 * c.kh + 17 * c.kw + 19 * c.stride + 23 * c.pad) % (2 ** 31 - 1)


def _ints(g, shape, lo=-VMAX, hi=VMAX):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def operands(c, float_pass=False):
    """dict of fp32 CPU tensors in the library's layouts: x (B,H,W,C), w [K][kh][kw][C], dy (B,OH,OW,K), bias (K), base (B,H,W,C),
    pro (4,C) BatchNorm block of the input channels, obn (4,K) of the output channels, res (B,OH,OW,K)."""
    g = torch.Generator().manual_seed(_seed(c) + (1 if float_pass else 0))
    oh, ow = out_size(c)
    o = {}
    if float_pass:
        o["x"] = torch.randn(c.B, c.H, c.W, c.C, generator=g)
        o["w"] = torch.randn(c.K, c.kh, c.kw, c.C, generator=g) / (c.C * c.kh * c.kw) ** 0.5
        o["dy"] = torch.randn(c.B, oh, ow, c.K, generator=g)
        o["bias"] = torch.randn(c.K, generator=g)
        o["base"] = torch.randn(c.B, c.H, c.W, c.C, generator=g)
        o["pro"] = torch.stack((torch.randn(c.C, generator=g) * 0.5, torch.rand(c.C, generator=g) + 0.5,
                                torch.randn(c.C, generator=g) * 0.3, torch.ones(c.C)))
        o["obn"] = torch.stack((torch.randn(c.K, generator=g) * 0.5, torch.rand(c.K, generator=g) + 0.5,
                                torch.randn(c.K, generator=g) * 0.3, torch.ones(c.K)))
        o["res"] = torch.randn(c.B, oh, ow, c.K, generator=g)
        return o
    o["x"] = _ints(g, (c.B, c.H, c.W, c.C))
    o["w"] = _ints(g, (c.K, c.kh, c.kw, c.C))
    o["dy"] = _ints(g, (c.B, oh, ow, c.K))
    o["bias"] = _ints(g, (c.K,))
    o["base"] = _ints(g, (c.B, c.H, c.W, c.C))
    pow2 = lambda n: torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (n,), generator=g)]
    o["pro"] = torch.stack((_ints(g, (c.C,), -2, 2), pow2(c.C), _ints(g, (c.C,), -2, 2), torch.ones(c.C)))
    o["obn"] = torch.stack((_ints(g, (c.K,)), pow2(c.K), _ints(g, (c.K,)), torch.ones(c.K)))
    o["res"] = _ints(g, (c.B, oh, ow, c.K))
    for k, t in o.items():
        assert bf16_exact(t), (c.name, k)
    act = ((o["x"] - o["pro"][0]) * o["pro"][1] + o["pro"][2]).clamp_min(0)
    assert bf16_exact(act) and float(act.abs().max()) <= PRO_MAX, c.name
    return o


def apply_pro(x64, pro):
    """The operand prologue: relu((x - mean) * scale + shift), BatchNorm block rows (mean, scale, shift, invstd)."""
    p = pro.double()
    return ((x64 - p[0]) * p[1] + p[2]).clamp_min(0)


def reference(c, o, pro=False):
    """fp64 F.conv2d and its autograd, in the library's layouts: dict y (no bias), dx (B,H,W,C), dw [K][kh][kw][C], db (K);
    with ``pro`` the operand is apply_pro(x) and dx is the gradient with respect to that operand."""
    xd = o["x"].double()
    if pro:
        xd = apply_pro(xd, o["pro"])
    xa = xd.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wd = o["w"].double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.conv2d(xa, wd, None, stride=c.stride, padding=c.pad)
    y.backward(o["dy"].double().permute(0, 3, 1, 2))
    return {"y": y.detach().permute(0, 2, 3, 1).contiguous(), "dx": xa.grad.permute(0, 2, 3, 1).contiguous(),
            "dw": wd.grad.permute(0, 2, 3, 1).contiguous(), "db": o["dy"].double().sum((0, 1, 2))}


def bnact_reference(y64, o, relu=True, residual=True):
    p = o["obn"].double()
    r = (y64 - p[0]) * p[1] + p[2]
    if residual:
        r = r + o["res"].double()
    return r.clamp_min(0) if relu else r


def unreached_mask(c):
    """(H, W) bool: input pixels that no (output pixel, tap) pair touches -- dx must be exactly 0 there."""
    oh, ow = out_size(c)

    def axis(n, k, no):
        hit = np.zeros(n, bool)
        for o_, r in itertools.product(range(no), range(k)):
            i = o_ * c.stride - c.pad + r
            if 0 <= i < n:
                hit[i] = True
        return hit
    return torch.from_numpy(~np.outer(axis(c.H, c.kh, oh), axis(c.W, c.kw, ow)))


def six_loops(c, o):
    """The definition, in plain loops over (output row, output column, filter row, filter column) with the batch / channel
    contractions as integer-exact numpy products: y, dx, dw in the library's layouts (float64)."""
    x, w, dy = (o[k].double().numpy() for k in ("x", "w", "dy"))
    oh, ow = out_size(c)
    y = np.zeros((c.B, oh, ow, c.K))
    dx = np.zeros_like(x)
    dw = np.zeros_like(w)
    for p in range(oh):
        for q in range(ow):
            for r in range(c.kh):
                for s in range(c.kw):
                    i, j = p * c.stride - c.pad + r, q * c.stride - c.pad + s
                    if not (0 <= i < c.H and 0 <= j < c.W):
                        continue
                    for b in range(c.B):
                        y[b, p, q] += w[:, r, s, :] @ x[b, i, j]
                        dx[b, i, j] += dy[b, p, q] @ w[:, r, s, :]
                        dw[:, r, s, :] += np.outer(dy[b, p, q], x[b, i, j])
    return {"y": torch.from_numpy(y), "dx": torch.from_numpy(dx), "dw": torch.from_numpy(dw)}


# ---------------------------------------------------------------------------------------------------------------------
# which kernel family the library must report (dpft_profile_get_family) -- restated from the dispatch rules of conv.hip
# ---------------------------------------------------------------------------------------------------------------------
N_CU = 256
X3_TILES = {(128, 128), (128, 64), (64, 64)}


def _split_on(mode):
    return mode in ("fp32+split", "bf16x3")


def _mfma_family(mode, big, multi_tap, tile):
    """Family of a vector-loader implicit-GEMM launch (forward, stride-1 or per-class data gradient)."""
    if mode == "bf16":
        return "bf16"
    if tile is None:
        return "x3" if (_split_on(mode) and multi_tap and big) else "f32"
    return "x3" if (mode == "bf16x3" and tuple(tile[:2]) in X3_TILES) else "f32"


def expected_family(c, kind, mode, tile=None, wtile=None, workspace=True):
    """mode: 'fp32' | 'fp32+split' | 'bf16x3' | 'bf16'; tile = (bm, bn, splits) of DPFT_FORCE_TILE; wtile = (tile, splits) of
    DPFT_FORCE_WGRAD."""
    oh, ow = out_size(c)
    taps = c.kh * c.kw
    unit = taps == 1 and c.stride == 1
    if kind == "fwd":
        if is_conv16(c) or c.C % 64:
            return "vector"
        return _mfma_family(mode, 2.0 * c.B * oh * ow * c.K * taps * c.C >= 2e9, not unit, tile)
    if kind == "dgrad":
        if is_conv16(c):
            return "vector"
        if c.C <= 4 and c.K % 4 == 0 and c.C * taps * c.K * 4 <= 40960:
            return "vector"
        if c.K % 64:
            return "vector"
        s = c.stride
        if s > 1:
            class_wgs = -(-(c.B * -(-c.H // s) * -(-c.W // s)) // 64) * -(-c.C // 64)
            if class_wgs >= N_CU // 2 or not workspace:
                launched = any((ph + c.pad) % s < c.kh and (pw + c.pad) % s < c.kw and ph < c.H and pw < c.W
                               for ph in range(s) for pw in range(s))
                return _mfma_family(mode, False, False, tile) if launched else "vector"
            return "f32"      # one launch over all taps: the fp32 kernel in every mode
        return _mfma_family(mode, 2.0 * c.B * c.H * c.W * c.C * taps * c.K >= 2e9, not unit, tile)
    assert kind == "wgrad"
    if workspace and (is_conv16(c) or is_thin1x1(c) or is_stem7(c)):
        return "vector"
    if c.C % 32 or c.K % 4:
        return "vector"
    bmn = 32 if c.K <= 32 else (128 if (c.K >= 128 and c.C >= 128 and -(-c.K // 128) * -(-c.C // 128) * taps >= 8) else 64)
    if wtile is not None:
        bmn = wtile[0]
    if mode == "bf16":
        return "bf16" if bmn in (64, 128) else "f32"
    m = c.B * oh * ow
    if bmn == 128 and _split_on(mode) and 2.0 * m * c.K * taps * c.C >= 2e9:
        return "x3"
    return "f32"
