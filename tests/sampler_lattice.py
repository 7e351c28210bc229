"""TEST INFRASTRUCTURE -- the sampling lattice of tests/test_sampler_rule.py (CPU) and tests/test_gpu_sampler_edges.py (GPU).

A bilinear sampler goes wrong where its rule has an edge: the border strips (-1 < t < 0, size-1 < t < size), the corners where two
strips meet, exact pixel positions (the location gradient jumps there), t = -1 and t = size (where the strict inequalities
decide), one-pixel-wide maps and the far outside.  Random locations hit those by chance or never; the lattice hits all of them by
construction: per level every pair (tx, ty) of quarter pixels from -2 to size + 2, plus +-2^20 pixels on each axis.

On power-of-two maps every intermediate of the kernels' own fp32 formulas is exact on this lattice, so the cell a sample falls
into is not a matter of rounding; ``replay_*`` recompute those formulas in numpy float32 and the tests assert bit equality."""
import numpy as np

POW2_SHAPES = [(1, 1), (1, 8), (4, 1), (2, 2), (8, 16), (32, 16)]       # (H, W)
ODD_SHAPES = [(13, 9), (7, 5), (3, 7)]
FAR = float(2 ** 20)


def axis_values(size, kinks=True):
    """Quarter pixels from -2 to size + 2 and +-2^20; ``kinks=False`` keeps the fractional parts .25 / .5 / .75 only."""
    t = np.arange(-8, 4 * (size + 2) + 1, dtype=np.float64) / 4
    if not kinks:
        t = t[t != np.floor(t)]
    return np.concatenate(([-FAR], t, [FAR])) if kinks else np.concatenate(([-FAR + 0.5], t, [FAR + 0.5]))


def level_points(H, W, kinks=True):
    """(n, 2) float64, columns (tx, ty): the full product of the two axes."""
    tx, ty = np.meshgrid(axis_values(W, kinks), axis_values(H, kinks), indexing="ij")
    return np.stack((tx.ravel(), ty.ravel()), -1)


def lattice_t(shapes, M=1, P=1, kinks=True):
    """Intended sample positions t (Q, M, L, P, 2) in pixels, (x, y) order.  One query per lattice point of the largest level;
    smaller levels repeat theirs; every (head, point) slot walks the same lattice from a different start, so each slot sees
    every point of every level."""
    pts = [level_points(H, W, kinks) for H, W in shapes]
    Q = max(len(p) for p in pts)
    t = np.empty((Q, M, len(shapes), P, 2), np.float64)
    q = np.arange(Q)
    for l, p in enumerate(pts):
        for m in range(M):
            for k in range(P):
                t[:, m, l, k] = p[(q + 977 * m + 3571 * k + 131 * l) % len(p)]
    return t


def sizes_wh(shapes):
    return np.array([[w, h] for h, w in shapes], np.float64)             # (L, 2) as (W, H)


def direct_loc(t, shapes):
    """loc = (t + 0.5) / size for kernels that take normalised locations; float32 (exact on power-of-two maps)."""
    return ((t + 0.5) / sizes_wh(shapes)[None, None, :, None, :]).astype(np.float32)


def replay_direct(loc32, shapes):
    """The generic operator's own arithmetic (msda.hip): h_im = loc * size - 0.5 in float32."""
    wh = sizes_wh(shapes).astype(np.float32)[None, None, :, None, :]
    return loc32.astype(np.float32) * wh - np.float32(0.5)


REF_GRID = np.array([0.0, 0.25, 0.5, 0.75, 1.0])


def ref_off_split(t, shapes):
    """For kernels that take ``ref + off / size``: a reference point per query from {0, .25, .5, .75, 1}^2 (shared by all levels,
    heads and points, as in the model) and the pixel offset that lands on t.  -> ref (Q, 2), off (Q, M, L, P, 2), float32."""
    Q = t.shape[0]
    q = np.arange(Q)
    ref = np.stack((REF_GRID[q % 5], REF_GRID[(q // 5) % 5]), -1)
    off = t + 0.5 - ref[:, None, None, None, :] * sizes_wh(shapes)[None, None, :, None, :]
    return ref.astype(np.float32), off.astype(np.float32)


def replay_ref_off(ref32, off32, shapes):
    """msda.hip / decoder_train_x.hip: lx = rx + ox / W; w_im = lx * W - 0.5, all float32.  ref (..., Q, 2) and
    off (..., Q, M, L, P, 2) with the same leading dimensions."""
    wh = sizes_wh(shapes).astype(np.float32)[:, None, :]
    loc = ref32.astype(np.float32)[..., None, None, None, :] + off32.astype(np.float32) / wh
    return loc * wh - np.float32(0.5)


def block_lattice(shapes, P, view, M=8):
    """The fused training block computes its offsets itself (sampling_offsets of the query); with a zero weight they are the
    bias, the same for every query, so there the lattice comes from the reference points, and per (head, level, point) a
    quarter-pixel offset pair from a list that reaches t = -1, t = size, both strips and the outside.  Two views share the work so
    that every float32 intermediate stays exact: view 0 walks refs on the 1/32 grid of [0, 1]^2 (ref * size is a whole or half
    pixel on every power-of-two map up to 16 wide) with its outside offsets at +-64 pixels; view 1 has them at +-2^20 pixels,
    where ``ref + off / size`` on a one-pixel map only holds multiples of 1/8, so its refs are the 1/8 grid, repeated.
    -> refs (1089, 2) float32, off (M, L, P, 2) float32."""
    n = 33 if view == 0 else 9
    g = np.arange(n, dtype=np.float64) / (n - 1)
    rx, ry = np.meshgrid(g, g, indexing="ij")
    refs = np.stack((rx.ravel(), ry.ravel()), -1)[np.arange(33 * 33) % (n * n)]
    far = 64.0 if view == 0 else FAR
    # with refs sweeping [0, 1], offset 0 on an axis walks that axis' low strip, interior and high strip on every map; -0.5 / +0.5
    # put ref 0 / ref 1 on t = -1 / t = size and the refs between on whole pixels
    pairs = [[(0, 0), (-0.5, 0), (0, -0.5), (0.5, 0), (0, 0.5), (-far, 0.75), (0.75, far), (-1.75, 1.25)],
             [(-0.5, -0.5), (0.5, 0.5), (-0.5, 0.5), (1.25, -1.75), (far, -far), (0.25, -0.25), (0, -far), (far, 0)]]
    off = np.empty((M, len(shapes), P, 2))
    for m in range(M):
        for l in range(len(shapes)):
            for p in range(P):
                off[m, l, p] = pairs[p % 2][(m + 3 * (p // 2) + l + view) % 8]
    return refs.astype(np.float32), off.astype(np.float32)


def block_t(refs, off, shapes):
    """Intended t (Q, M, L, P, 2), float64, of ``block_lattice``."""
    return (refs.astype(np.float64)[:, None, None, None, :] * sizes_wh(shapes)[None, None, :, None, :]
            + off.astype(np.float64)[None] - 0.5)


ZONES = ("below", "low strip", "interior", "high strip", "above")


def block_shapes(P):
    """The fused block takes at most 20 (level, point) slots per head: five maps at P = 4, all six below."""
    return POW2_SHAPES[:5] if P == 4 else POW2_SHAPES


def zone(t, size):
    """Per axis: 0 t <= -1 | 1 -1 < t < 0 | 2 0 <= t <= size-1 | 3 size-1 < t < size | 4 t >= size."""
    t = np.asarray(t, np.float64)
    return np.where(t <= -1, 0, np.where(t < 0, 1, np.where(t <= size - 1, 2, np.where(t < size, 3, 4))))


def assert_coverage(t, shapes, kinks=True, far=FAR, what=""):
    """t (..., L, P, 2): every level has samples in each of the 9 inside zones (low strip / interior / high strip per axis) and
    outside; with ``kinks`` also on t = -1, t = size and an integer t of each axis while the other axis is inside."""
    t = np.asarray(t, np.float64)
    L = len(shapes)
    t = np.moveaxis(t, -3, 0).reshape(L, -1, 2)
    for l, (H, W) in enumerate(shapes):
        zx, zy = zone(t[l, :, 0], W), zone(t[l, :, 1], H)
        for a in (1, 2, 3):
            for b in (1, 2, 3):
                assert np.any((zx == a) & (zy == b)), f"{what} level {l} {(H, W)}: no sample with x in {ZONES[a]}, y in {ZONES[b]}"
        x_in, y_in = (zx >= 1) & (zx <= 3), (zy >= 1) & (zy <= 3)
        for a in (0, 4):
            assert np.any((zx == a) & y_in) and np.any((zy == a) & x_in), f"{what} level {l} {(H, W)}: nothing {ZONES[a]} the map"
        assert np.any(np.abs(t[l]) >= far), f"{what} level {l}: no far-outside sample"
        if kinks:
            for ax, size, other in ((0, W, y_in), (1, H, x_in)):
                ta = t[l, :, ax]
                for name, hit in (("t = -1", ta == -1), ("t = size", ta == size),
                                  ("integer t inside", (ta == np.floor(ta)) & (ta >= 0) & (ta <= size - 1))):
                    assert np.any(hit & other), f"{what} level {l} {(H, W)} axis {ax}: no sample on {name}"
