"""TEST INFRASTRUCTURE -- the lattice of tests/test_head_lattice.py (CPU) and tests/test_gpu_head_lattice.py (GPU).

The TRAINING decoder's view reduction + detection head + reference points (dpft_amd/csrc/decoder_train_h.hip: hd_train_fwd_kernel,
hd_train_bwd_kernel, ref_points_bwd_kernel, through train_fused.head_block / reference_points / RefPointsFn) in front of the fp64
oracle (oracle.dprt_oracle: F.linear reduction, detection_head, reference_points, autograd) at the sizes, forms and points where
such a block goes wrong:

  * sizes: V in {1, 2, 3, 4} (at V = 4 every lane of the staged y3 is live and the reduction order k * V + v fills HR_Y3C),
    1 / 2 / 15 / 16 classes, B Q in {1, 3, 4, 5, 63, 64} (one live wave of four, every remainder, a full last block), B >= 2;
  * forms: 3- and 4-row projections, int64 shape rows of stride 2 and 3 read in place, int32 and mixed-stride shapes that
    _Proj compacts, flags all 0 / all 1 / mixed, and a different T, P and (H, W) with H != W for every (batch element, view);
  * reference-point rows PLACED, not drawn: strictly inside, clipped below / above in u and in v, un / vn exactly 0 and exactly 1
    (the clip passes the gradient there), w == 0, r == 0, rho == 0 above and below, the negative x axis (+-180 degrees), and
    elevations of 80, 85, 89, 89.9 and 89.99 degrees.  The head adds its output to prev_center, so prev_center is the wanted
    centre minus the fp64 head output; the cases with exact points zero the centre branch's last weight, which makes
    center == prev_center bit for bit, and use transformations (signed permutations, dyadic shifts) and centres on a 2^-14
    grid that fp32 applies without rounding.

The reference-point gradient also stands here in closed form (``ref_points_grad_closed``), with the well-conditioned elevation
term  d el / d t = (180 / pi) / r^2 * (-tz tx / rho, -tz ty / rho, rho)  and the conventions of the kernel: no contribution at
all at r == 0, none through azimuth and elevation at rho == 0.  It equals the oracle's autograd wherever that is finite
(tests/test_head_lattice.py); on the rows at or above 89 degrees and on the axis, where autograd in fp32 loses every digit or
is NaN, it IS the reference, and its float32 evaluation is the yardstick.

No GPU code here.  ``python -m tests.head_lattice`` prints the table; ``python -m tests.head_lattice seeds`` searches the seeds."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from tests.decoder_lattice import distance, tolerance  # noqa: F401  (the rule: 1e-4 |ref| + 1e-5 max|ref|, elementwise)

OUT_NAMES = ("x", "center", "size", "angle", "class", "refs")
BRANCHES = ("center", "size", "angle", "class")
GRAD_NAMES = ("y3", "prev", "red_w") + tuple(f"{b}.{k}" for b in BRANCHES for k in (0, 3, 6))
ALL = frozenset(OUT_NAMES)
GRID = 2.0 ** -14                                   # exact cases: centres on this grid, |coordinate| < 2^9
STEEP = (80.0, 85.0, 89.0, 89.9, 89.99)
CLOSED_FROM = 89.0                                  # rows at or above: the closed form is the reference
AUTOGRAD_BELOW = 85.0                               # rows below: the closed form must equal the oracle's autograd
# signed permutations (rows): what fp32 applies exactly
PERMS = (((1, 0, 0), (0, 1, 0), (0, 0, 1)), ((0, 1, 0), (-1, 0, 0), (0, 0, 1)), ((0, 0, 1), (0, 1, 0), (-1, 0, 0)),
         ((1, 0, 0), (0, 0, -1), (0, 1, 0)), ((0, 0, -1), (1, 0, 0), (0, -1, 0)), ((0, -1, 0), (0, 0, 1), (-1, 0, 0)))
# steep rows: (range, azimuth in rad, sign of the elevation) by row index
STEEP_ROWS = ((30.0, 0.3, 1), (24.0, 2.0, -1), (40.0, -1.2, 1), (20.0, -2.8, -1), (36.0, 1.0, 1))

# kinds of a view: "plain" (flag 0; dyadic affine map, w = 1), "persp" (flag 0; w = 1 + z / 8), "spher" (flag 1; a general affine
# T, (r, azimuth, elevation) mapped into the unit square wherever the centre lies), "axis" (flag 1; T a signed permutation with
# a dyadic shift, both projection rows weigh the elevation), "elev" (the same without a weight on the azimuth: on a steep row the
# azimuth's gradient grows as 1 / rho while the elevation's stays at 1 / r, and would hide it under the rule's absolute term)
# rows: (class, view) placed at the head of every batch element's rows; the other rows are "inside"
Case = namedtuple("Case", "name B Q kinds ncls p_rows shapes rows exact seed why")

CASES = [
    Case("generic-v3", 2, 32, ("plain", "spher", "persp"), 2, (4, 3, 3), "i64s3",
         (("u-below", 0), ("u-above", 0), ("v-below", 0), ("v-above", 0)), False, 1000,
         "B Q = 64: a full last block; mixed flags; stride-3 shape rows in place; both sides of the clip in u and v"),
    Case("v4-c16", 3, 21, ("spher", "plain", "spher", "persp"), 16, (3, 4, 4, 3), "i64s2",
         (("u-above", 1), ("v-below", 1)), False, 2002,
         "V = 4: every y3 lane live, HR_Y3C full; 16 classes; B Q = 63 = 3 mod 4; B = 3"),
    Case("v1-c1", 1, 1, ("plain",), 1, (3,), "i64s2", (), False, 3000, "one row: one live wave of four; V = 1; one class; flags all 0"),
    Case("v2-c15", 1, 5, ("spher", "spher"), 15, (4, 4), "i32", (), False, 4000,
         "B Q = 5 = 1 mod 4; 15 classes; flags all 1; int32 shapes (compacted)"),
    Case("edges", 2, 5, ("plain", "axis"), 2, (3, 4), "mixed", (("u0", 0), ("u1", 0), ("v0", 0), ("v1", 0)), True, 5000,
         "un / vn exactly 0 and 1 with a slope behind; mixed shape strides (compacted); B Q = 10 = 2 mod 4"),
    Case("poles", 2, 8, ("axis", "persp", "plain"), 2, (3, 3, 4), "i64s3",
         (("r0", 0), ("axis-up", 0), ("axis-down", 0), ("negx0", 0), ("negx+", 0), ("negx-", 0), ("wzero", 1)), True, 6000,
         "r == 0, rho == 0 above and below, the +-180 degree cut, w == 0; B = 2"),
    Case("el-80", 1, 3, ("elev",), 2, (3,), "i64s2", (("el80", 0),) * 3, True, 7000, "elevation +-80 degrees; B Q = 3"),
    Case("el-85", 2, 2, ("elev", "elev"), 2, (4, 3), "i64s2", (("el85", 0), ("el85", 1)), True, 8000,
         "elevation +-85 degrees in either view; B Q = 4: one full block"),
    Case("el-89", 1, 5, ("elev",), 2, (4,), "i64s3", (("el89", 0),) * 5, True, 9000, "elevation +-89 degrees"),
    Case("el-89.9", 2, 2, ("elev",), 2, (3,), "i64s2", (("el89.9", 0),) * 2, True, 10000, "elevation +-89.9 degrees; B = 2"),
    Case("el-89.99", 1, 4, ("elev",), 2, (3,), "i64s2", (("el89.99", 0),) * 4, True, 11000,
         "elevation +-89.99 degrees: 1 - (tz / r)^2 is below the fp32 rounding of tz / r"),
]
EXACT_CLASSES = ("u0", "u1", "v0", "v1", "r0", "axis-up", "axis-down", "negx0", "negx+", "negx-", "wzero")


def by_name(name):
    return next(c for c in CASES if c.name == name)


def case_id(c):
    return c.name


def n_views(c):
    return len(c.kinds)


def flags_of(c):
    return tuple(int(k in ("spher", "axis", "elev")) for k in c.kinds)


def image(v, b):
    """(H, W) of view v for batch element b: all different, H != W."""
    return 96 + 16 * v + 8 * b, 160 - 24 * v + 4 * b


def plain_offsets(v, b):
    return 0.5 + b / 16 + v / 32, 0.25 + b / 32 + v / 16          # un = x / 64 + ou, vn = y / 32 + z / 128 + ov


def steep_of(cls):
    return float(cls[2:]) if cls.startswith("el") else None


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _projection(c, v, b, g):
    """(T (4,4), P (p_rows,4)) of view v, batch element b, in fp64 (rounded to fp32 by the caller)."""
    kind, (H, W) = c.kinds[v], image(v, b)
    T = torch.zeros(4, 4, dtype=torch.float64)
    P = torch.zeros(4, 4, dtype=torch.float64)
    P[2, 3] = P[3, 3] = 1.0
    if kind == "plain":
        ou, ov = plain_offsets(v, b)
        P[0, 0], P[0, 3] = W / 64, W * ou
        P[1, 1], P[1, 2], P[1, 3] = H / 32, H / 128, H * ov
    elif kind == "persp":
        gain = 0.008 * (1 + b / 8)
        P[0, 0], P[0, 2], P[0, 3] = W * gain, W / 16, W / 2          # u = W (gain x + w / 2), w = 1 + z / 8
        P[1, 1], P[1, 2], P[1, 3] = H * gain, H / 16, H / 2
        P[2, 2] = 0.125
    elif kind == "spher":
        T[:3, :3] = torch.eye(3, dtype=torch.float64) + 0.05 * torch.randn(3, 3, generator=g, dtype=torch.float64)
        T[:3, 3] = torch.randn(3, generator=g, dtype=torch.float64)
        T[3, 3] = 1.0
        P[0, 0], P[0, 3] = W / 100 * (1 + b / 16), W * 0.1           # r
        P[1, 1], P[1, 2], P[1, 3] = H / 720, H / 1800, H * (0.5 + b / 64)
        if v % 2:
            P[2, 0] = 0.002                                          # w = 1 + 0.002 r
    else:                                                            # axis, elev
        T[:3, :3] = torch.tensor(PERMS[(b + 3 * v) % len(PERMS)], dtype=torch.float64)
        T[:3, 3] = torch.tensor([b + 1.0, -2.0 + v, 0.5 * (v + 1)], dtype=torch.float64)
        T[3, 3] = 1.0
        P[0, 0], P[0, 2], P[0, 3] = W / 128, W / 720, W * (0.25 + b / 128)
        P[1, 2], P[1, 3] = -H / 450, H * 0.5
        if kind == "axis":
            P[1, 1] = H / 720
        else:                                                        # no azimuth: its 1 / rho gradient would bury the elevation's
            P[1, 0] = H / 256
    return T, P[:c.p_rows[v]]


def _snap(t):
    return torch.round(t / GRID) * GRID


def _place(c, cls, v, b, q, g, proj):
    """The centre of row (b, q) of class ``cls`` in view v, fp64."""
    rnd = lambda lo, hi: lo + (hi - lo) * float(torch.rand((), generator=g, dtype=torch.float64))   # noqa: E731
    el = steep_of(cls)
    if cls == "inside" or cls in ("u-below", "u-above", "v-below", "v-above"):
        pv = v if cls != "inside" else next((i for i, k in enumerate(c.kinds) if k == "plain"), None)
        if pv is None:
            out = torch.tensor([rnd(5, 40), rnd(-15, 15), rnd(-3, 5)], dtype=torch.float64)
        else:
            ou, ov = plain_offsets(pv, b)
            un = {"u-below": rnd(-0.4, -0.2), "u-above": rnd(1.2, 1.4)}.get(cls, rnd(0.15, 0.85))
            vn = {"v-below": rnd(-0.4, -0.2), "v-above": rnd(1.2, 1.4)}.get(cls, rnd(0.15, 0.85))
            z = rnd(-3, 5)
            out = torch.tensor([64 * (un - ou), 32 * (vn - ov - z / 128), z], dtype=torch.float64)
        return _snap(out) if c.exact else out
    if cls in ("u0", "u1", "v0", "v1"):
        assert c.kinds[v] == "plain" and c.exact
        ou, ov = plain_offsets(v, b)
        x, y, z = 12.0 - b, 3.0 + b, 2.0                              # inside in the other coordinate
        if cls[0] == "u":
            x = 64 * (float(cls[1]) - ou)
        else:
            z = 4.0
            y = 32 * (float(cls[1]) - ov - z / 128)
        return torch.tensor([x, y, z], dtype=torch.float64)
    if cls == "wzero":
        assert c.kinds[v] == "persp" and c.exact
        return torch.tensor([20.0 - b, 15.0 + b, -8.0], dtype=torch.float64)
    assert c.kinds[v] in ("axis", "elev") and c.exact, (c.name, cls)
    T = proj[v][b][0]
    if el is not None:
        r, az, sign = STEEP_ROWS[(q + b) % len(STEEP_ROWS)]
        rho = r * math.cos(math.radians(el))
        t = torch.tensor([rho * math.cos(az), rho * math.sin(az), sign * r * math.sin(math.radians(el))], dtype=torch.float64)
    else:
        t = torch.tensor({"r0": (0.0, 0.0, 0.0), "axis-up": (0.0, 0.0, 4.0 + b), "axis-down": (0.0, 0.0, -4.5 - b),
                          "negx0": (-5.5 - b, 0.0, 1.5), "negx+": (-5.0, 2.0 ** -12, 1.0 + b),
                          "negx-": (-7.0 - b, -2.0 ** -12, -2.0)}[cls], dtype=torch.float64)
    return T[:3, :3].T @ (_snap(t) - T[:3, 3])                       # exact: a signed permutation and a dyadic shift


def row_classes(c):
    """[(b, q, class, view)] of every row; view is None for "inside"."""
    out = []
    for b in range(c.B):
        for q in range(c.Q):
            cls, v = c.rows[q] if q < len(c.rows) else ("inside", None)
            out.append((b, q, cls, v))
    return out


def make_inputs(c, seed=None):
    """fp32 CPU inputs of a case: y3 (V,B,Q,16), prev (B,Q,3), weights [13] in train_fused.head_params order, T / P per view,
    hw [(B,2) int64] and the same rows in the case's form (shape), flags, the six cotangents gys, the wanted centres."""
    seed = c.seed if seed is None else seed
    g = torch.Generator().manual_seed(seed)
    B, Q, V = c.B, c.Q, n_views(c)
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    y3 = (randn(V, B, Q, 16) * 0.8).float()
    weights = [(randn(16, 16 * V) * 1.5 / math.sqrt(16 * V)).float()]
    for name, nout in zip(BRANCHES, (3, 3, 2, c.ncls)):
        weights += [(randn(16, 16) * 0.4).float(), (randn(16, 16) * 0.4).float(), (randn(nout, 16) * 0.3).float()]
    if c.exact:
        weights[3].zero_()                                            # center_head.6: center == prev_center bit for bit
    proj = [[_projection(c, v, b, g) for b in range(B)] for v in range(V)]
    T = [torch.stack([proj[v][b][0] for b in range(B)]).float() for v in range(V)]
    P = [torch.stack([proj[v][b][1] for b in range(B)]).float() for v in range(V)]
    target = torch.zeros(B, Q, 3, dtype=torch.float64)
    for b, q, cls, v in row_classes(c):
        target[b, q] = _place(c, cls, v, b, q, g, proj)
    # prev_center = wanted centre - the fp64 head's centre output
    x = F.linear(torch.stack(list(y3.double()), dim=-1).reshape(B, Q, -1), weights[0].double())
    h = F.relu(F.linear(F.relu(F.linear(x, weights[1].double())), weights[2].double()))
    prev = (target - F.linear(h, weights[3].double())).float()
    if c.exact:
        assert torch.equal(prev.double(), target), c.name             # the grid is fp32's
    hw = [torch.tensor([image(v, b) for b in range(B)], dtype=torch.int64) for v in range(V)]
    wide = lambda s: torch.cat((s, torch.full((B, 1), 3, dtype=torch.int64)), 1)   # noqa: E731
    if c.shapes == "i64s2":
        shape = list(hw)
    elif c.shapes == "i64s3":
        shape = [wide(s) for s in hw]
    elif c.shapes == "i32":
        shape = [s.to(torch.int32) for s in hw]
    else:
        assert c.shapes == "mixed" and V >= 2
        shape = [wide(s) if v % 2 else s for v, s in enumerate(hw)]
    sizes = [(B, Q, 16), (B, Q, 3), (B, Q, 3), (B, Q, 2), (B, Q, c.ncls), (V, B, Q, 2)]
    gys = [randn(*s).float() for s in sizes]
    gys[5] *= 256.0          # d refs / d center is about 1 / 64 to 1 / 400 per unit: with this the reference points' term in
                             # d prev_center is as large as the centre's own cotangent and cannot hide under it
    return dict(y3=y3, prev=prev, weights=weights, T=T, P=P, hw=hw, shape=shape, flags=flags_of(c), gys=gys, target=target)


def oracle_T(inp, v, dtype):
    """The oracle reads the flag off `transformation.any()`: an all-zero T for a view without one."""
    return inp["T"][v].to(dtype) if inp["flags"][v] else torch.zeros_like(inp["T"][v], dtype=dtype)


# ---------------------------------------------------------------------------------------------------------------------
# the reference points in closed form
# ---------------------------------------------------------------------------------------------------------------------
def geometry(center, T, P, hw, flag):
    """Per row, in center's dtype: dict(un, vn (before the clip), w, and for a flagged view tx, ty, tz, r, rho, az, el in degrees)."""
    k = 180.0 / math.pi
    out = {}
    if flag:
        t = torch.einsum("bij,bqj->bqi", T[:, :3, :3], center) + T[:, None, :3, 3]
        tx, ty, tz = t.unbind(-1)
        rho2 = tx * tx + ty * ty
        r = torch.sqrt(rho2 + tz * tz)
        pos = r > 0
        el = torch.asin(torch.where(pos, tz / torch.where(pos, r, torch.ones_like(r)), torch.zeros_like(r))) * k
        az = torch.atan2(ty, tx) * k
        s = torch.stack((r, az, el), -1)
        out.update(tx=tx, ty=ty, tz=tz, r=r, rho=torch.sqrt(rho2), rho2=rho2, az=az, el=el)
    else:
        s = center
    p = torch.einsum("bij,bqj->bqi", P[:, :3, :3], s) + P[:, None, :3, 3]
    w = p[..., 2]
    nz = w != 0
    safe = torch.where(nz, w, torch.ones_like(w))
    H, W = hw[:, 0:1].to(center.dtype), hw[:, 1:2].to(center.dtype)
    out.update(u_=p[..., 0], v_=p[..., 1], w=w, un=torch.where(nz, p[..., 0] / safe, p[..., 0]) / W,
               vn=torch.where(nz, p[..., 1] / safe, p[..., 1]) / H, H=H, W=W)
    return out


def ref_points_grad_closed(center, T, P, hw, flag, drefs):
    """d (sum refs * drefs) / d center of ONE view in closed form, in center's dtype: (B,Q,3).  The clip passes the gradient on
    [0, 1] closed; w == 0 takes the undivided coordinates; at r == 0 the view adds nothing; at rho == 0 azimuth and elevation
    add nothing; elsewhere  d el / d t = (180 / pi) / r^2 (-tz tx / rho, -tz ty / rho, rho)."""
    k = 180.0 / math.pi
    m = geometry(center, T, P, hw, flag)
    zero = torch.zeros_like(m["un"])
    du1 = torch.where((m["un"] >= 0) & (m["un"] <= 1), drefs[..., 0] / m["W"], zero)
    dv1 = torch.where((m["vn"] >= 0) & (m["vn"] <= 1), drefs[..., 1] / m["H"], zero)
    nz = m["w"] != 0
    safe = torch.where(nz, m["w"], torch.ones_like(zero))
    du_, dv_ = torch.where(nz, du1 / safe, du1), torch.where(nz, dv1 / safe, dv1)
    dw = torch.where(nz, -(du1 * m["u_"] + dv1 * m["v_"]) / (safe * safe), zero)
    ds = [P[:, None, 0, j] * du_ + P[:, None, 1, j] * dv_ + P[:, None, 2, j] * dw for j in range(3)]
    if not flag:
        return torch.stack(ds, -1)
    tx, ty, tz, r, rho, rho2 = (m[n] for n in ("tx", "ty", "tz", "r", "rho", "rho2"))
    one = torch.ones_like(zero)
    pr, ph = r > 0, rho2 > 0
    sr, sh, sh2 = torch.where(pr, r, one), torch.where(ph, rho, one), torch.where(ph, rho2, one)
    g0 = torch.where(pr, ds[0] / sr, zero)
    ga = torch.where(ph, ds[1] * k / sh2, zero)
    ge = torch.where(ph, ds[2] * k / (sr * sr), zero)
    dt = torch.stack((g0 * tx - ga * ty - ge * tz * tx / sh, g0 * ty + ga * tx - ge * tz * ty / sh, g0 * tz + ge * rho), -1)
    return torch.einsum("bij,bqi->bqj", T[:, :3, :3], dt)


def closed_rows(c, inp):
    """(B,Q) bool: rows whose reference-point gradient is the closed form's -- on the vertical axis or at the origin of a
    flagged view (autograd of atan2 / asin is not finite), or at an elevation of 89 degrees or more."""
    center = cached(c)["out64"][1]
    rows = torch.zeros(c.B, c.Q, dtype=torch.bool)
    for v, f in enumerate(inp["flags"]):
        if f:
            m = geometry(center, inp["T"][v].double(), inp["P"][v].double(), inp["hw"][v], 1)
            rows |= (m["rho"] == 0) | (m["el"].abs() >= CLOSED_FROM)
    return rows


# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------
def state_dict(weights, dtype):
    sd = {"mp.reduction_layer.weight": weights[0].to(dtype)}
    for g, name in enumerate(BRANCHES):
        for k, layer in enumerate((0, 3, 6)):
            sd[f"hd.layers.{name}_head.{layer}.weight"] = weights[1 + 3 * g + k].to(dtype)
    return sd


def _forward(c, inp, dtype, leaves=False):
    from oracle import dprt_oracle as O
    B, Q = c.B, c.Q
    leaf = (lambda t: t.to(dtype).requires_grad_(True)) if leaves else (lambda t: t.to(dtype))
    y3, prev, weights = leaf(inp["y3"]), leaf(inp["prev"]), [leaf(w) for w in inp["weights"]]
    sd = state_dict(weights, dtype)
    x = F.linear(torch.stack(list(y3), dim=-1).reshape(B, Q, -1), sd["mp.reduction_layer.weight"])
    o = O.detection_head(x, prev, sd, "hd")
    return y3, prev, weights, sd, x, o


def _oracle_refs(c, inp, center, dtype):
    from oracle import dprt_oracle as O
    return torch.stack([O.reference_points(center, oracle_T(inp, v, dtype), inp["P"][v].to(dtype), inp["hw"][v].to(dtype))
                        for v in range(n_views(c))])


def reference(c, inp, dtype=torch.float64, present=ALL, use_closed=None):
    """The oracle in ``dtype`` on the CPU -> dict(outs [6], grads [15] for the cotangents named in ``present``, g_auto / g_closed:
    the reference points' gradient to the centre by autograd and in closed form).  On the rows of ``use_closed`` (B,Q) the closed
    form replaces autograd before the head's backward, so that a NaN of the axis never reaches a weight gradient."""
    y3, prev, weights, sd, x, o = _forward(c, inp, dtype, leaves=True)
    cen = o["center"].detach().requires_grad_(True)
    refs = _oracle_refs(c, inp, cen, dtype)
    gys = [g.to(dtype) for g in inp["gys"]]
    (g_auto,) = torch.autograd.grad(refs, cen, gys[5])
    g_closed = sum(ref_points_grad_closed(cen.detach(), inp["T"][v].to(dtype), inp["P"][v].to(dtype), inp["hw"][v],
                                          inp["flags"][v], gys[5][v]) for v in range(n_views(c)))
    outs = [x, o["center"], o["size"], o["angle"], o["class"]]
    cot = [g if n in present else torch.zeros_like(g) for n, g in zip(OUT_NAMES, gys[:5])]
    if "refs" in present:
        g_ref = g_auto if use_closed is None else torch.where(use_closed.unsqueeze(-1), g_closed, g_auto)
        cot[1] = cot[1] + g_ref
    grads = torch.autograd.grad(outs, [y3, prev] + weights, cot)
    return dict(outs=[t.detach() for t in outs] + [refs.detach()], grads=[t.detach() for t in grads], g_auto=g_auto, g_closed=g_closed)


_CACHE, _REFS = {}, {}


def cached(c):
    """dict(inp, out64 [6]) of a case, once per process."""
    if c.name not in _CACHE:
        inp = make_inputs(c)
        with torch.no_grad():
            _, _, _, _, x, o = _forward(c, inp, torch.float64)
            refs = _oracle_refs(c, inp, o["center"], torch.float64)
        _CACHE[c.name] = dict(inp=inp, out64=[x, o["center"], o["size"], o["angle"], o["class"], refs])
    return _CACHE[c.name]


def cached_reference(c, dtype=torch.float64, present=ALL):
    """``reference`` with the closed form on ``closed_rows``, once per (case, dtype, present) and left unchanged."""
    key = (c.name, dtype, present)
    if key not in _REFS:
        inp = cached(c)["inp"]
        _REFS[key] = reference(c, inp, dtype, present, closed_rows(c, inp))
    return _REFS[key]


# ---------------------------------------------------------------------------------------------------------------------
# the input conditions, on the fp64 reference alone
# ---------------------------------------------------------------------------------------------------------------------
def check_inputs(c, inp=None):
    """-> dict of figures; raises AssertionError when the case's inputs would let an error hide or a row is not in its class."""
    fig = {}
    if inp is None:
        inp = cached(c)["inp"]
    with torch.no_grad():
        _, _, _, sd, x, o = _forward(c, inp, torch.float64)
        refs = _oracle_refs(c, inp, o["center"], torch.float64)
    # 1. no ReLU input at zero
    pre = []
    for name in BRANCHES:
        p0 = F.linear(x, sd[f"hd.layers.{name}_head.0.weight"])
        p3 = F.linear(F.relu(p0), sd[f"hd.layers.{name}_head.3.weight"])
        pre += [p0.flatten(), p3.flatten()]
        if name == "size":
            pre.append(F.linear(F.relu(p3), sd["hd.layers.size_head.6.weight"]).flatten())
    pre = torch.cat(pre)
    fig["preact_min_over_max"] = float(pre.abs().min() / pre.abs().max())
    assert fig["preact_min_over_max"] > 1e-5, (c.name, "a ReLU input at zero", fig["preact_min_over_max"])
    # 2. every output is far above the absolute term of the rule
    for n, t in zip(OUT_NAMES, [x, o["center"], o["size"], o["angle"], o["class"], refs]):
        fig["max_" + n] = float(t.abs().max())
        assert fig["max_" + n] >= 0.1, (c.name, n, fig["max_" + n])
    # 3. the rows are what they claim, and nothing else sits at an edge
    center = o["center"]
    geo = [geometry(center, inp["T"][v].double(), inp["P"][v].double(), inp["hw"][v], f) for v, f in enumerate(inp["flags"])]
    exact_uv = {}                                   # (view, b, q, "un" | "vn") -> 0.0 | 1.0
    count = {}
    planned = {"wzero": set(), "r0": set(), "rho0": set(), "steep": set()}
    for b, q, cls, v in row_classes(c):
        count[cls] = count.get(cls, 0) + 1
        m = None if v is None else geo[v]
        at = lambda n: float(m[n][b, q])            # noqa: E731
        el = steep_of(cls)
        if cls == "inside":
            continue
        if cls in ("u-below", "u-above", "v-below", "v-above"):
            mine, other = ("un", "vn") if cls[0] == "u" else ("vn", "un")
            assert (at(mine) < -0.1) if cls.endswith("below") else (at(mine) > 1.1), (c.name, b, q, cls, at(mine))
            assert 0.1 < at(other) < 0.9, (c.name, b, q, cls, at(other))
        elif cls in ("u0", "u1", "v0", "v1"):
            mine, other = ("un", "vn") if cls[0] == "u" else ("vn", "un")
            assert at(mine) == float(cls[1]) and 0.1 < at(other) < 0.9, (c.name, b, q, cls, at(mine), at(other))
            slope = inp["P"][v][b, 0, 0] if cls[0] == "u" else inp["P"][v][b, 1, 1]
            assert float(slope) != 0 and float(inp["gys"][5][v, b, q, 0 if cls[0] == "u" else 1]) != 0
            exact_uv[(v, b, q, mine)] = float(cls[1])
        elif cls == "wzero":
            assert at("w") == 0 and 0.05 < at("un") < 0.95 and 0.05 < at("vn") < 0.95, (c.name, b, q, at("w"), at("un"), at("vn"))
            planned["wzero"].add((v, b, q))
        elif cls == "r0":
            assert at("r") == 0, (c.name, b, q, at("r"))
            planned["r0"].add((v, b, q))
            planned["rho0"].add((v, b, q))
        elif cls in ("axis-up", "axis-down"):
            assert at("rho") == 0 and (at("tz") > 0) == (cls == "axis-up") and abs(at("el")) == 90, (c.name, b, q, cls)
            planned["rho0"].add((v, b, q))
        elif cls.startswith("negx"):
            assert at("tx") < 0 and abs(at("az")) > 179.9, (c.name, b, q, cls, at("az"))
            assert {"negx0": at("ty") == 0 and at("az") == 180, "negx+": at("ty") > 0 and at("az") < 180,
                    "negx-": at("ty") < 0 and at("az") > -180 and at("az") < 0}[cls], (c.name, b, q, cls, at("ty"), at("az"))
        else:
            assert el is not None, cls
            off = 90 - abs(at("el"))
            assert abs(off - (90 - el)) <= 0.1 * (90 - el), (c.name, b, q, cls, at("el"))
            planned["steep"].add((v, b, q))
    fig["rows"] = count
    if steep_rows := [cls for _, _, cls, _ in row_classes(c) if steep_of(cls) is not None]:
        signs = {float(geo[v]["tz"][b, q]) > 0 for b, q, cls, v in row_classes(c) if steep_of(cls) is not None}
        assert signs == {True, False} and len(steep_rows) >= 2, (c.name, "both signs of the elevation", signs)
    near = 0
    for v, m in enumerate(geo):
        for n in ("un", "vn"):
            t = m[n]
            edge = ((t.abs() < 1e-6) | ((t - 1).abs() < 1e-6)).nonzero().tolist()
            for b, q in edge:
                assert exact_uv.get((v, b, q, n)) == float(t[b, q]), (c.name, "an unplanned point at a clip edge", v, b, q, n, float(t[b, q]))
                near += 1
        got = {(v, b, q) for b, q in (m["w"] == 0).nonzero().tolist()}
        assert got == {k for k in planned["wzero"] if k[0] == v}, (c.name, "w == 0 rows", v, got)
        if inp["flags"][v]:
            got = {(v, b, q) for b, q in (m["r"] == 0).nonzero().tolist()}
            assert got == {k for k in planned["r0"] if k[0] == v}, (c.name, "r == 0 rows", v, got)
            got = {(v, b, q) for b, q in (m["rho"] == 0).nonzero().tolist()}
            assert got == {k for k in planned["rho0"] if k[0] == v}, (c.name, "rho == 0 rows", v, got)
            got = {(v, b, q) for b, q in ((m["el"].abs() >= 75) & (m["rho"] > 0)).nonzero().tolist()}
            assert got == {k for k in planned["steep"] if k[0] == v}, (c.name, "steep rows", v, got)
    assert near == len(exact_uv), (c.name, near, len(exact_uv))
    fig["exact_edge_points"] = near
    if c.exact:
        assert torch.equal(center, inp["prev"].double()), c.name
    fig["inside"] = float(torch.stack([((m["un"] > 0) & (m["un"] < 1) & (m["vn"] > 0) & (m["vn"] < 1)).double().mean() for m in geo]).mean())
    fig["exempt_rows"] = 0                           # every row of every case is compared
    return fig


def find_seed(c, tries=200):
    """The first seed from the case's base (a multiple of 1000) whose inputs meet ``check_inputs``."""
    base = c.seed - c.seed % 1000
    for seed in range(base, base + tries):
        try:
            check_inputs(c, make_inputs(c, seed))
            return seed
        except AssertionError:
            continue
    raise AssertionError((c.name, "no seed"))


def table_rows():
    rows = []
    for c in CASES:
        special = ",".join(dict.fromkeys(cls for cls, _ in c.rows)) or "-"
        rows.append(f"{c.name:11s} B={c.B} Q={c.Q:2d} V={n_views(c)} ncls={c.ncls:2d} {'/'.join(c.kinds):24s} P rows {c.p_rows} "
                    f"shapes {c.shapes:6s} rows {special}: {c.why}")
    return rows


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["seeds"]:
        for case in CASES:
            print(case.name, case.seed, "->", find_seed(case))
    else:
        print("\n".join(table_rows()))
