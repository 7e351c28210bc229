"""fp64 torch-autograd restatement of the criterion's GIoU3D term (dpft_amd/csrc/giou_loss.hip) and the pair
lattice its tests share.

    term = w / B * sum_b 1 / P_b * sum_k (1 - G(pred[b, i_k], gt[b, j_k])) / 2          P_b matched pairs (i_k, j_k)

G: BEV corners -> Sutherland-Hodgman clip -> shoelace area, times the z overlap; union = v1 + v2 - vol ALWAYS (the matcher
keeps the reference's union = 0 for disjoint boxes); the enclosing box over all sixteen corners with torch min / max;
yaw = atan2(sin, cos) differentiated through (zero gradient at sin = cos = 0).  An invalid box (a size <= 0 or
min(lw, lh, wh) / 2 <= 1e-4) gives G = -1 with a zero gradient.  Control flow looks at values only, like the kernel's.

Every lattice value is rounded to fp32 first, so the kernel and this file see the same numbers.
"""
import numpy as np
import torch

F64 = torch.float64


def box_valid(size) -> bool:
    l, w, h = (float(v) for v in (size.detach() if isinstance(size, torch.Tensor) else size))
    return l > 0 and w > 0 and h > 0 and min(l * w, l * h, w * h) / 2 > 1e-4


def _yaw(angle):
    s, c = angle[0], angle[1]
    if float(s.detach()) == 0.0 and float(c.detach()) == 0.0:
        return (s + c) * 0.0                     # atan2(0, 0) = 0, no gradient
    return torch.atan2(s, c)


def _bev_corners(center, size, yaw):
    co, si = torch.cos(yaw), torch.sin(yaw)
    pts = []
    for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1)):      # counter-clockwise for l, w > 0
        x, y = size[0] * (sx / 2), size[1] * (sy / 2)
        pts.append((co * x - si * y + center[0], si * x + co * y + center[1]))
    return pts


def _area2(poly):
    a = 0.0
    for k in range(len(poly)):
        (x1, y1), (x2, y2) = poly[k], poly[(k + 1) % len(poly)]
        a = a + (x1 * y2 - x2 * y1)
    return a


def _clip(poly, q):
    """Convex counter-clockwise ``poly`` clipped by the half-planes of the convex counter-clockwise ``q``."""
    for e in range(len(q)):
        (ax, ay), (bx, by) = q[e], q[(e + 1) % len(q)]
        inp, poly = poly, []
        if not inp:
            break
        for k in range(len(inp)):
            (cx, cy), (dx, dy) = inp[k], inp[(k + 1) % len(inp)]
            sc = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
            sd = (bx - ax) * (dy - ay) - (by - ay) * (dx - ax)
            if float(sc.detach()) >= 0:
                poly.append((cx, cy))
            if (float(sc.detach()) >= 0) != (float(sd.detach()) >= 0):
                t = sc / (sc - sd)
                poly.append((cx + t * (dx - cx), cy + t * (dy - cy)))
    return poly


def giou_pair(center, size, angle, g_center, g_size, g_angle, parts=None):
    """G of one pair; fp64 tensors (3), (3), (2) each.  ``parts`` (a dict) receives vol, v1, v2, evol as floats."""
    if not (box_valid(size) and box_valid(g_size)):
        return (center.sum() + size.sum() + angle.sum()) * 0.0 - 1.0
    A = _bev_corners(center, size, _yaw(angle))
    Q = _bev_corners(g_center, g_size, _yaw(g_angle))
    xs = torch.stack([p[0] for p in A + Q])
    ys = torch.stack([p[1] for p in A + Q])
    azl, azh = center[2] - size[2] / 2, center[2] + size[2] / 2
    bzl, bzh = g_center[2] - g_size[2] / 2, g_center[2] + g_size[2] / 2
    evol = (xs.max() - xs.min()) * (ys.max() - ys.min()) * (torch.max(azh, bzh) - torch.min(azl, bzl))
    poly = _clip(A, Q)
    inter = torch.abs(_area2(poly)) / 2 if len(poly) >= 3 else torch.zeros((), dtype=F64)
    dz = torch.min(azh, bzh) - torch.max(azl, bzl)
    vol = inter * dz if float(dz.detach()) > 0 else inter * 0.0
    v1, v2 = size.prod(), g_size.prod()
    union = v1 + v2 - vol
    if parts is not None:
        parts.update(vol=float(vol.detach()), v1=float(v1.detach()), v2=float(v2.detach()), evol=float(evol.detach()),
                     vertices=len(poly))
    return vol / union - (evol - union) / evol


# ----------------------------------------------------------------------------------------------------------------- lattice
def _pair(name, center, size, angle, g_center, g_size, g_angle):
    r = lambda v: np.asarray(v, dtype=np.float32).astype(np.float64)      # rounded to fp32 first
    return {"name": name, "center": r(center), "size": r(size), "angle": r(angle), "g_center": r(g_center),
            "g_size": r(g_size), "g_angle": r(g_angle)}


_GT = dict(g_center=(1.2, 0.5, 0.4), g_size=(3.5, 1.8, 1.6), g_angle=(-0.3, 0.9))
_PRED = dict(center=(0.3, -0.2, 0.1), size=(4.0, 2.0, 1.5), angle=(0.5, 0.8))

NAMED = [
    _pair("partial_overlap", **_PRED, **_GT),
    _pair("disjoint_bev", **_PRED, g_center=(8.0, 6.0, 0.2), g_size=(3.5, 1.8, 1.6), g_angle=(-0.3, 0.9)),
    _pair("disjoint_z_only", **_PRED, g_center=(1.2, 0.5, 5.0), g_size=(3.5, 1.8, 1.6), g_angle=(-0.3, 0.9)),
    _pair("pred_inside_target", center=(1.1, 0.4, 0.3), size=(1.0, 0.8, 0.5), angle=(0.4, 0.7),
          g_center=(1.2, 0.5, 0.4), g_size=(5.0, 4.0, 3.0), g_angle=(-0.3, 0.9)),
    _pair("target_inside_pred", center=(1.2, 0.5, 0.4), size=(5.0, 4.0, 3.0), angle=(-0.3, 0.9),
          g_center=(1.1, 0.4, 0.3), g_size=(1.0, 0.8, 0.5), g_angle=(0.4, 0.7)),
    _pair("eight_vertices", center=(0.05, -0.03, 0.07), size=(2.0, 2.1, 1.0), angle=(0.05, 1.0),
          g_center=(0.0, 0.0, 0.0), g_size=(2.05, 1.95, 1.2), g_angle=(0.7314, 0.6820)),
    _pair("unnormalised_angle", center=(0.3, -0.2, 0.1), size=(4.0, 2.0, 1.5), angle=(0.2, -0.55), **_GT),
    _pair("zero_angle", center=(0.3, -0.2, 0.1), size=(4.0, 2.0, 1.5), angle=(0.0, 0.0), **_GT),
    _pair("negative_size", center=(0.3, -0.2, 0.1), size=(-2.0, 2.0, 1.5), angle=(0.5, 0.8), **_GT),
    _pair("tiny_size", center=(0.3, -0.2, 0.1), size=(3.0, 2.0, 1e-5), angle=(0.5, 0.8), **_GT),
]
INVALID = {"negative_size", "tiny_size"}


def random_pairs(n, seed=0):
    """centres U(-3, 3), sizes U(0.5, 5), (sin, cos) ~ N(0, 1)^2 -- for both boxes of a pair."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        c, s, a = rng.uniform(-3, 3, (2, 3)), rng.uniform(0.5, 5, (2, 3)), rng.standard_normal((2, 2))
        out.append(_pair(f"random_{k}", c[0], s[0], a[0], c[1], s[1], a[1]))
    return out


N_RANDOM = 64
LATTICE = NAMED + random_pairs(N_RANDOM)


def tensors(p, requires_grad=False):
    t = [torch.tensor(p[k], dtype=F64) for k in ("center", "size", "angle", "g_center", "g_size", "g_angle")]
    for v in t[:3]:
        v.requires_grad_(requires_grad)
    return t


def pair_value_and_grad(p, parts=None):
    """(G, d G / d (center 3 | size 3 | angle 2)) of a lattice pair by autograd."""
    t = tensors(p, requires_grad=True)
    G = giou_pair(*t, parts=parts)
    G.backward()
    return float(G.detach()), torch.cat([v.grad for v in t[:3]]).numpy()


def pair_numeric_grad(p, h=1e-6):
    """Central differences of G over the eight inputs."""
    base = np.concatenate([p["center"], p["size"], p["angle"]])
    out = np.zeros(8)
    for i in range(8):
        vals = []
        for sgn in (1.0, -1.0):
            x = base.copy()
            x[i] += sgn * h
            q = dict(p, center=x[:3], size=x[3:6], angle=x[6:])
            vals.append(float(giou_pair(*tensors(q))))
        out[i] = (vals[0] - vals[1]) / (2 * h)
    return out


# ------------------------------------------------------------------------------------------------------------------ tables
def pack(pairs_per_sample, N, Mmax, seed=0):
    """Lattice pairs -> the tensors the entries read.  ``pairs_per_sample``: one list of pairs per sample (its matched
    count).  Queries sit at random distinct rows, unmatched rows hold random valid boxes, unmatched slots hold -1, unused
    target rows hold unit boxes.  fp32 / int32 CPU tensors; ``where[b][k] = (query row, pair)``."""
    rng = np.random.default_rng(seed)
    B = len(pairs_per_sample)
    center = rng.uniform(-3, 3, (B, N, 3)).astype(np.float32)
    size = rng.uniform(0.5, 5, (B, N, 3)).astype(np.float32)
    angle = rng.standard_normal((B, N, 2)).astype(np.float32)
    gt_box = np.zeros((B, Mmax, 8), dtype=np.float32)
    gt_box[..., 3:6] = 1.0
    gt_box[..., 7] = 1.0
    match = np.full((B, Mmax, 2), -1, dtype=np.int32)
    counts = np.zeros(B, dtype=np.int32)
    where = []
    for b, pairs in enumerate(pairs_per_sample):
        assert len(pairs) <= min(N, Mmax)
        rows, cols = rng.permutation(N)[:len(pairs)], rng.permutation(Mmax)[:len(pairs)]
        counts[b] = len(pairs)
        where.append([(int(i), p) for i, p in zip(rows, pairs)])
        for k, (i, j, p) in enumerate(zip(rows, cols, pairs)):
            center[b, i], size[b, i], angle[b, i] = p["center"], p["size"], p["angle"]
            gt_box[b, j] = np.concatenate([p["g_center"], p["g_size"], p["g_angle"]])
            match[b, k] = (i, j)
    t = {k: torch.from_numpy(v) for k, v in dict(center=center, size=size, angle=angle, gt_box=gt_box, match=match,
                                                  counts=counts).items()}
    t["where"] = where
    return t


def table_reference(t, w, total_in=0.0):
    """fp64 reference of a packed table: G (B,Mmax) (nan in empty slots), term, total, d term / d (center, size, angle)."""
    center, size, angle = (t[k].double().clone().requires_grad_(True) for k in ("center", "size", "angle"))
    gt = t["gt_box"].double()
    B, Mmax = gt.shape[:2]
    G = torch.full((B, Mmax), float("nan"), dtype=F64)
    term = torch.zeros((), dtype=F64)
    for b in range(B):
        P = int(t["counts"][b])
        for k in range(P):
            i, j = (int(v) for v in t["match"][b, k])
            g = giou_pair(center[b, i], size[b, i], angle[b, i], gt[b, j, :3], gt[b, j, 3:6], gt[b, j, 6:])
            G[b, k] = g.detach()
            term = term + (1 - g) / 2 / P
    term = term * (w / B)
    if term.requires_grad:
        term.backward()
    zero = lambda v: v.grad if v.grad is not None else torch.zeros_like(v)
    term = term.detach()
    return {"G": G, "term": float(term), "total": float(total_in) + float(term), "dcenter": zero(center), "dsize": zero(size),
            "dangle": zero(angle)}
