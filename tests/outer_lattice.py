"""TEST INFRASTRUCTURE -- the shape lattice of tests/test_outer_lattice.py (CPU) and tests/test_gpu_rows_outer.py (GPU).

dpft_rows_outer_f32 produces every weight and bias gradient of the training decoder:
out[g][off + a * n_b + b] = sum_r rows[g][r][col_a + a] * rows[g][r][col_b + b] for a list of (col_a, n_a, col_b, n_b, off) specs
(col_b < 0: column sums, the b operand is 1).  The model's own call has 13 specs and 83 output tiles; it takes the compact grid,
the 16-byte vector loads (and the scalar loop only for its n_a == 2 specs), full b-tiles and R = 1600.  The lattice walks what
that call never reaches: the dense fallback grid (a spec above 255 tiles, a launch above 192), the scalar loop for each of its
four causes, partial a- and b-tiles, R on either side of the 64 row groups, an output stride with unwritten gaps, 40 specs.

Operands of the exact pass are integers in [-4, 4]: every product is an integer of magnitude <= 16 and every partial sum of every
summation order stays below 16 * R < 2^24, exactly representable in fp32 -- fused or not, whatever the order, the kernel must
return the fp64 result BIT FOR BIT.

No GPU code here: the case list, the operands, the fp64 reference (one einsum per spec), a restatement of the host dispatch of
dpft_rows_outer_f32 and of rows_outer_kernel's vector predicate, and the map of the output floats a spec writes."""
import zlib
from collections import namedtuple

import numpy as np
import torch

VMAX = 4                              # |operand| <= 4 in the exact pass
MAX_SPECS = 40                        # OUTER_MAX_SPECS
MAX_TILES = 192                       # OUTER_MAX_TILES: tiles of a compact launch
MAX_SPEC_TILES = 255                  # tile index of the compact grid is one byte
TILE = 16
ROW_GROUPS = 64                       # row groups of a block: a thread's chain is ceil(R / 64) rows
FLOATS_MAX = 12_000_000               # G * R * W of a case

NA_VALUES = [1, 2, 15, 16, 17, 31, 32, 480]
NB_VALUES = [1, 15, 16, 17, 32, 33]
COLSUM_NA_VALUES = [1, 16, 17, 640]
R_VALUES = [1, 63, 64, 65, 130, 1600, 4099]
G_VALUES = [1, 3]
PATHS = ["vec", "scalar:col_a", "scalar:W", "scalar:na", "scalar:base"]
GRID_MODES = ["compact", "dense:spec", "dense:total"]

# specs: tuple of (col_a, n_a, col_b, n_b, out_off); ptr_off: offset of the `rows` pointer from a 16-byte boundary, in floats
Case = namedtuple("Case", "name G R W specs out_gstride ptr_off")
Dispatch = namedtuple("Dispatch", "mode grid surplus_blocks base_aligned paths")


def cdiv(a, b):
    return -(-a // b)


def spec_floats(s):
    return s[1] * (1 if s[2] < 0 else s[3])


def spec_tiles(s):
    return cdiv(s[1], TILE) * cdiv(s[3], TILE)


def packed(cols, gap=0, start=0):
    """(col_a, n_a, col_b, n_b) list -> specs with consecutive output offsets (``gap`` unwritten floats between them)."""
    out, off = [], start
    for ca, na, cb, nb in cols:
        out.append((ca, na, cb, nb, off))
        off += na * (1 if cb < 0 else nb) + gap
    return tuple(out), off - gap


def make_case(name, G, R, W, cols, gap=0, start=0, stride_extra=0, ptr_off=0):
    specs, floats = packed(cols, gap, start)
    c = Case(name, G, R, W, specs, floats + stride_extra, ptr_off)
    assert 1 <= len(specs) <= MAX_SPECS and G >= 1 and R >= 1 and W >= 1 and ptr_off in (0, 1), c
    for ca, na, cb, nb, off in specs:
        assert na >= 1 and ca >= 0 and ca + na <= W and off >= 0, (name, ca, na)
        assert (nb == 1) if cb < 0 else (nb >= 1 and cb + nb <= W), (name, cb, nb)
    assert G * R * W <= FLOATS_MAX, c
    check_exactness(c)
    return c


def check_exactness(c):
    """|a|, |b| <= 4: products <= 16, any partial sum of any order <= 16 * R -- an integer below 2^24, exact in fp32."""
    assert VMAX * VMAX * c.R < 2 ** 24, c
    return True


# ---------------------------------------------------------------------------------------------------------------------
# the model's own call (XattnFfnBlocksFn.backward): the row layout of the cross-attention + FFN block's backward
# ---------------------------------------------------------------------------------------------------------------------
XR = dict(DLIN=0, DF=480, DPRE=496, DOUT=528, G3=544, B3=560, G2=576, B2=592, DBV=608, DVEC=624, QP=640, HD=656, Y2=688, VEC=704,
          SAMP=720, FLOATS=848)


def model_xattn_cols():
    X = XR
    cols = [(0, X["QP"], -1, 1),
            (X["DLIN"], X["DF"] - X["DLIN"], X["QP"], 16),
            (X["DF"], X["DPRE"] - X["DF"], X["HD"], 32),
            (X["DPRE"], X["DOUT"] - X["DPRE"], X["Y2"], 16),
            (X["DOUT"], X["G3"] - X["DOUT"], X["VEC"], 16)]
    cols += [(X["DVEC"] + 2 * m, 2, X["SAMP"] + 16 * m, 16) for m in range(8)]
    return cols


def _specs40_cols():
    cols = [(4 * (i % 3), 1 + i % 20, 40 + i % 5, 1 + (i * 7) % 33) for i in range(40)]
    assert sum(spec_tiles((ca, na, cb, nb, 0)) for ca, na, cb, nb in cols) <= MAX_TILES
    return cols


def build_lattice():
    nb = NB_VALUES
    cases = [
        # the model's own call: 13 specs, 83 tiles, compact grid
        make_case("model-xattn", 3, 1600, XR["FLOATS"], model_xattn_cols()),
        # dense grid because ONE spec has 256 tiles (tile index does not fit the compact table's byte)
        make_case("dense-spec256", 1, 70, 512, [(0, 256, 256, 256)]),
        # dense grid because the launch has 216 tiles: 30 + 40 + 100 + 6 + 40; max_tiles = 100, so the blocks of four of the five
        # specs run past their own tile count and must return
        make_case("dense-total", 3, 65, 704, [(0, 480, 480, 16), (0, 640, -1, 1), (0, 160, 160, 160), (16, 33, 64, 17),
                                              (0, 320, 320, 32)]),
        # n_a x n_b: every pair, a-operand at a vector-friendly column (n_a = 17, 31: full first a-tile + partial second one)
        make_case("sweep-na-le16", 3, 63, 96, [(0, a, 48, b) for a in (1, 2, 15, 16) for b in nb]),
        make_case("sweep-na-gt16", 1, 130, 96, [(0, a, 48, b) for a in (17, 31, 32) for b in nb]),
        make_case("na480-nb33", 1, 64, 520, [(0, 480, 480, 33)]),
        # column sums
        make_case("colsums", 1, 65, 640, [(0, 1, -1, 1), (16, 16, -1, 1), (32, 17, -1, 1), (0, 640, -1, 1)]),
        # R below one pass of the 64 row groups, and far above
        make_case("R1", 3, 1, 64, [(0, 32, 32, 17), (0, 5, -1, 1)]),
        make_case("R4099-overlap", 1, 4099, 48, [(0, 32, 16, 32), (0, 32, 0, 32)]),
        # scalar loop because col_a % 4 != 0 (W % 4 == 0, aligned base; full and partial a-tiles, partial b-tiles)
        make_case("col-a-odd", 1, 65, 64, [(2, 16, 32, 16), (5, 32, 7, 17), (2, 31, 40, 15), (1, 16, -1, 1)]),
        # scalar loop because W % 4 != 0.  R * W % 4 == 2: the base of g = 1 is 8 bytes off a 16-byte boundary, g = 0 and 2 are on one
        make_case("W50-g3", 3, 65, 50, [(0, 16, 16, 16), (0, 32, 32, 18), (4, 16, -1, 1)]),
        make_case("W49-g3", 3, 63, 49, [(0, 16, 16, 33), (8, 17, -1, 1)]),
        # scalar loop because of the base ALONE: rows pointer one float past a 16-byte boundary, W % 4 == 0, col_a % 4 == 0
        make_case("ptr-off1", 3, 64, 64, [(0, 16, 16, 16), (0, 32, -1, 1), (16, 17, 0, 33)], ptr_off=1),
        make_case("ptr-off1-R4099", 1, 4099, 32, [(0, 16, 16, 16)], ptr_off=1),
        # out_gstride above the floats written, gaps between the specs, first spec not at 0
        make_case("gaps", 3, 65, 48, [(0, 16, 16, 16), (0, 17, -1, 1), (16, 2, 32, 15)], gap=37, start=3, stride_extra=101),
        # a Gram spec (col_a == col_b, n_a == n_b), partly overlapping column blocks
        make_case("gram", 3, 130, 64, [(0, 32, 0, 32), (0, 32, 16, 32), (4, 17, 4, 17)]),
        # the table limit
        make_case("specs40", 1, 64, 96, _specs40_cols()),
    ]
    seen = set()
    for c in cases:
        assert c.name not in seen, c.name
        seen.add(c.name)
    return cases


def by_name(name):
    return next(c for c in LATTICE if c.name == name)


# ---------------------------------------------------------------------------------------------------------------------
# dispatch: the host code of dpft_rows_outer_f32 and the `vec` predicate of rows_outer_kernel, restated
# ---------------------------------------------------------------------------------------------------------------------
def grid_mode(c):
    """'compact' (one block per existing tile), or the dense (max_tiles, n_specs, G) grid with the reason the host code meets
    first: 'dense:spec' (a spec above 255 tiles) or 'dense:total' (more than 192 tiles so far)."""
    nt = 0
    for s in c.specs:
        t = spec_tiles(s)
        if t > MAX_SPEC_TILES:
            return "dense:spec"
        if nt + t > MAX_TILES:
            return "dense:total"
        nt += t
    return "compact"


def tile_path(c, s, a_tile, g):
    """The loop a block of a-tile ``a_tile`` of spec ``s`` takes for group ``g``: 'vec', or 'scalar:<cause>' with the first
    failing term of the kernel's predicate, in its order (col_a, W, na, base)."""
    if s[0] % 4:
        return "scalar:col_a"
    if c.W % 4:
        return "scalar:W"
    if min(TILE, s[1] - a_tile * TILE) != TILE:
        return "scalar:na"
    if not base_aligned(c, g):
        return "scalar:base"
    return "vec"


def base_aligned(c, g):
    """rows + g * R * W on a 16-byte boundary (the allocation itself is)."""
    return (c.ptr_off + g * c.R * c.W) % 4 == 0


def dispatch(c):
    mode = grid_mode(c)
    tiles = [spec_tiles(s) for s in c.specs]
    if mode == "compact":
        grid, surplus = (sum(tiles), 1, c.G), 0
    else:
        grid = (max(tiles), len(c.specs), c.G)
        surplus = sum(max(tiles) - t for t in tiles) * c.G        # blocks that take the `ti >= ta * tb` return
    paths = {(si, at, g): tile_path(c, s, at, g)
             for si, s in enumerate(c.specs) for at in range(cdiv(s[1], TILE)) for g in range(c.G)}
    return Dispatch(mode, grid, surplus, [base_aligned(c, g) for g in range(c.G)], paths)


def covered_mask(c, spec=None):
    """bool (G * out_gstride): the floats of `out` the call writes (``spec``: that spec alone)."""
    m = np.zeros((c.G, c.out_gstride), bool)
    for si, s in enumerate(c.specs):
        if spec is None or si == spec:
            m[:, s[4]:s[4] + spec_floats(s)] = True
    return m.reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------
# operands and the fp64 reference
# ---------------------------------------------------------------------------------------------------------------------
def _seed(c):
    return zlib.crc32(c.name.encode())


def operands(c, float_pass=False):
    """rows (G, R, W) fp32: integers in [-4, 4], or standard normal for the float pass."""
    g = torch.Generator().manual_seed(_seed(c) + (1 if float_pass else 0))
    if float_pass:
        return torch.randn(c.G, c.R, c.W, generator=g)
    return torch.randint(-VMAX, VMAX + 1, (c.G, c.R, c.W), generator=g).float()


def reference(rows, c, absolute=False):
    """fp64 (G * out_gstride): one einsum per spec, 0 where nothing is written.  ``absolute``: sum_r |a_r * b_r| instead (the
    scale of the float pass's error bound).  `+ 0.0` turns a -0.0 of a one-term product into the +0.0 that a sum started at +0.0
    gives in round-to-nearest."""
    x = rows.double().reshape(c.G, c.R, c.W)
    if absolute:
        x = x.abs()
    out = torch.zeros(c.G, c.out_gstride, dtype=torch.float64)
    for ca, na, cb, nb, off in c.specs:
        a = x[:, :, ca:ca + na]
        if cb < 0:
            v = torch.einsum("gra->ga", a)
        else:
            v = torch.einsum("gra,grb->gab", a, x[:, :, cb:cb + nb])
        out[:, off:off + na * (1 if cb < 0 else nb)] = v.reshape(c.G, -1) + 0.0
    return out.reshape(-1)


def triple_loop(rows, c):
    """The definition in plain Python loops (tiny cases only)."""
    x = rows.double().reshape(c.G, c.R, c.W).tolist()
    out = [0.0] * (c.G * c.out_gstride)
    for g in range(c.G):
        for ca, na, cb, nb, off in c.specs:
            for a in range(na):
                for b in range(1 if cb < 0 else nb):
                    t = 0.0
                    for r in range(c.R):
                        t += x[g][r][ca + a] * (1.0 if cb < 0 else x[g][r][cb + b])
                    out[g * c.out_gstride + off + a * (1 if cb < 0 else nb) + b] = t
    return torch.tensor(out, dtype=torch.float64)


LATTICE = build_lattice()
