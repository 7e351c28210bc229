"""TEST INFRASTRUCTURE -- the geometry lattice of tests/test_decoder_lattice.py (CPU) and tests/test_gpu_decoder_lattice.py (GPU).

The fused INFERENCE decoder (dpft_amd/csrc/decoder.hip: decoder_scores_head_kernel and its several-trip form
decoder_scores_head_long_kernel, decoder_xattn_kernel<7>, decoder_xattn_last_kernel<7>, the pack kernels) was only ever run at the product's geometry, Q = 400, 5 levels x 4 points, 4
iterations, 2 classes, 3 views.  The lattice puts it in front of the fp64 oracle (oracle.dprt_oracle.impfusion) at the sizes where
such kernels go wrong:

  * the score kernel's chunk (QC = 50 queries per block, a query PAIR per thread) and slice (NS = 10 key slices) edges: Q % QC in
    {0, 1, QC - 1}, odd Q, Q < NS (empty slices merged through -inf partials), Q = 1, and Q past the 512 items one staging trip
    covers (462 / 463 / 512 / 1000);
  * the soft-max against the Cauchy-Schwarz bound: slices whose every term underflows (den < 2^-100) are redone in two-pass form,
    alone (scores-uniform: packed and composed rows) and merged with ordinary slices, one query of a pair only (scores-split);
  * row tails: B Q % 7 (waves without a row, which in the fused last launch still take part in the ticket hand-over), B Q % 4;
  * iters = 1 (no fused last launch, no partial rows, a trailing head-only launch) and iters = 2 (the ticket-zeroing launch is
    directly followed by the last one);
  * the slot table: L P < 20, different L / P per view, P in {1, 2, 3}; levels of one pixel, one row or one column; V = 4;
    1 and 16 classes;
  * projection forms: `transformation.any()` left to the device vs given, an all-zero T, 3 and 4 projection rows, w == 0,
    shape rows read in place with a stride other than 2.

No GPU code here: the case table, the modules and inputs of a case (seeded; built so that the comparison means something -- see
``check_inputs``), the fp64 / fp32 reference with its reference points and sampling locations recorded, and the first layer's
attention output before out_proj.  ``python -m tests.decoder_lattice`` prints the table."""
import math
from collections import OrderedDict, namedtuple
from contextlib import contextmanager

import torch

LEVELS = ((6, 5), (3, 3), (2, 1), (1, 4), (1, 1))                     # (H, W) of pyramid level l, every view
IMAGES = ((64, 96), (128, 43), (37, 107), (50, 50))                   # (H, W) the reference points are normalised by, per view
KINDS = ("plain", "transformed", "perspective", "plain")              # projection of view v
BOX = ((5.0, 60.0), (-15.0, 15.0), (-2.0, 4.0))                       # center0 is uniform in this box (x, y, z)
RTOL, ATOL_SCALE = 1e-4, 1e-5                                         # the rule of test_product_fuser_forward_matches_reference_golden
KEYS = ("center", "size", "angle", "class")                           # "center" is compared as center - center0

Case = namedtuple("Case", "name B Q LP iters ncls seed special why")   # LP: ((L, P) per view)

CASES = [
    Case("anchor", 2, 100, ((5, 4),) * 3, 4, 2, 24, "", "the product's slot table off Q = 400; B Q % 7 = 4"),
    Case("q1", 1, 1, ((1, 1),), 2, 1, 2, "", "one key, nine empty slices, clipped pair partner, 1 live wave of 7, 1 head row of 4"),
    Case("below-slices", 3, 7, ((5, 4), (1, 1), (3, 2), (2, 3)), 1, 16, 3, "",
         "Q < NS; V = 4; mixed slot counts; iters = 1; 16 classes; 1-pixel and 1-wide levels"),
    Case("chunk-49", 1, 49, ((2, 2), (4, 1)), 2, 2, 4, "", "one short chunk whose last pair has a clipped partner; iters = 2"),
    Case("chunk-50", 1, 50, ((2, 2), (4, 1)), 2, 2, 5, "", "exactly one chunk"),
    Case("chunk-51", 1, 51, ((2, 2), (4, 1)), 2, 2, 6, "", "a last chunk holding one query"),
    Case("odd-101", 2, 101, ((5, 3), (3, 4)), 3, 3, 7, "", "odd Q; B Q % 7 = 6; B Q % 4 = 2; three-point slots"),
    Case("batch-5", 5, 50, ((5, 4),), 2, 2, 8, "", "Bsa = 1 in the first layer against B = 5 later"),
    Case("q462", 1, 462, ((2, 2),), 2, 2, 9, "", "the last Q that one staging trip covers"),
    Case("q463", 1, 463, ((2, 2),) * 2, 2, 2, 10, "", "one key past the first staging trip"),
    Case("q512", 1, 512, ((2, 2),), 2, 2, 11, "", "the query rows start the second staging trip"),
    Case("q1000", 1, 1000, ((2, 2),), 2, 2, 12, "", "three staging trips"),
    Case("scores-uniform", 2, 60, ((2, 2),) * 2, 2, 2, 13, "uniform", "fallback slices alone, packed and composed rows"),
    Case("scores-split", 1, 60, ((2, 2),), 1, 2, 14, "split", "fallback slices merged with ordinary ones; one query of a pair"),
    Case("forms", 2, 37, ((3, 2),) * 3, 2, 2, 15, "clamped", "projection and shape forms; clamped reference points"),
    Case("w-zero", 1, 20, ((2, 2),), 1, 2, 16, "wzero", "w == 0 exactly for some queries"),
]
STAGING = 512                      # items (keys + the chunk's queries) one staging trip of a score block covers: up to it
                                   # decoder_scores_head_kernel runs, above it decoder_scores_head_long_kernel
SPLIT_AT = 31                      # scores-split: keys / queries below it point one way, the others the opposite way
FALLBACK_HEAD = 0                  # the head the score cases bend
FORMS = ("none", "flags", "p4", "shape-stride3", "shape-int32")


def by_name(name):
    return next(c for c in CASES if c.name == name)


def case_id(c):
    return c.name


def n_views(c):
    return len(c.LP)


def limits():
    """(QC, NS, XR, largest admitted Q) from the library (host code: no GPU needed)."""
    import ctypes as C
    from dpft_amd.hip.lib import lib
    out = (C.c_int32 * 4)()
    lib.call("dpft_decoder_limits", out)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------
# modules
# ---------------------------------------------------------------------------------------------------------------------
def fuser_config(c):
    from dpft_amd.configs import load_config
    cfg = load_config("kradar")
    comp, m = cfg["computing"], cfg["model"]
    V = n_views(c)
    fcfg = dict(comp | m["fuser"])
    fcfg.update(n_queries=c.Q, m_views=V, n_levels=[l for l, _ in c.LP], n_points=[p for _, p in c.LP], n_heads=[8] * V,
                i_iter=c.iters, dropout=0.0)
    hcfg = dict(comp | m["head"])
    hcfg.update(num_classes=c.ncls)
    return m, fcfg, hcfg


# gains of the last head layer per branch: with the default init the heads answer ~0.05 against a center0 of ~35
HEAD_GAIN = {"center": 12.0, "size": 4.0, "angle": 4.0, "class": 4.0}


def make_fuser(c):
    """IMPFusion + LinearDetectionHead of the case on the CPU, seeded: default init + N(0, 0.05) on every parameter, sampling
    offsets of about half a pixel (the maps are a few pixels wide), head and reduction weights scaled so that the outputs are
    far above the absolute term of the tolerance; the score cases bend one head's q / k rows."""
    from dpft_amd.models.fusers import build_fuser
    from dpft_amd.models.heads import build_head
    m, fcfg, hcfg = fuser_config(c)
    torch.manual_seed(1000 + c.seed)
    head = build_head(m["head"]["name"], hcfg)
    fuser = build_fuser(m["fuser"]["name"], fcfg, head=head)
    g = torch.Generator().manual_seed(2000 + c.seed)
    with torch.no_grad():
        for name, p in fuser.named_parameters():
            p.add_(torch.randn(p.shape, generator=g) * 0.05)
            if name.endswith("sampling_offsets.bias"):
                p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 2.4)
            elif name.endswith("sampling_offsets.weight"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.04)
            elif name.endswith("attention_weights.weight") or name.endswith("attention_weights.bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
            elif name.endswith("reduction_layer.weight"):
                p.mul_(2.0)
            elif "_head." in name:
                branch = name.split(".layers.")[1].split("_head.")[0]
                p.mul_(HEAD_GAIN[branch] if name.endswith(".6.weight") else 1.5)
        if c.special == "uniform":
            # every score of the head is -81 sqrt(2) log2(e) = -165.3 in the exp2 domain against a bound of +165.3
            h = FALLBACK_HEAD
            for layer in fuser.mpfusion.values():
                for ml in layer.ml_fusion_layers.values():
                    w, b = ml.self_attn.in_proj_weight, ml.self_attn.in_proj_bias
                    w[2 * h:2 * h + 2] = 0.0
                    w[16 + 2 * h:16 + 2 * h + 2] = 0.0
                    b[2 * h:2 * h + 2] = 9.0
                    b[16 + 2 * h:16 + 2 * h + 2] = -9.0
        elif c.special == "split":
            # channel 0 of query + position is +-(1 + a little) by key; the head's q and k rows read that channel alone, times
            # 9: aligned pairs score about +165 in the exp2 domain, opposed ones about -165
            h = FALLBACK_HEAD
            sign = torch.where(torch.arange(c.Q) < SPLIT_AT, 1.0, -1.0)
            fuser.query[:, 0] = 0.0
            fuser.query_embedding.weight[:, 0] = sign * (1.0 + 0.02 * torch.rand(c.Q, generator=g))
            for ml in fuser.mpfusion["fusion0"].ml_fusion_layers.values():
                w, b = ml.self_attn.in_proj_weight, ml.self_attn.in_proj_bias
                for r in (2 * h, 2 * h + 1, 16 + 2 * h, 16 + 2 * h + 1):
                    w[r] = 0.0
                    w[r, 0] = 9.0
                    b[r] = 0.0
    return fuser.eval()


def state_dict64(fuser, dtype=torch.float64):
    return {"f." + k: v.detach().cpu().to(dtype) for k, v in fuser.state_dict().items()}


def oracle_cfg(c):
    return {"i_iter": c.iters, "n_heads": [8] * n_views(c), "n_points": [p for _, p in c.LP], "activation": "Mish"}


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _affine(lo_in, hi_in, lo_out, hi_out):
    """(gain, offset) of the map [lo_in, hi_in] -> [lo_out, hi_out]."""
    gain = (hi_out - lo_out) / (hi_in - lo_in)
    return gain, lo_out - gain * lo_in


def make_inputs(c):
    """fp32 CPU inputs of a case: dict(views=[OrderedDict level -> (B,H,W,16)], shape=[(B,2) int64 H, W], projection=[(T (B,4,4),
    P (B,3,4))], center0 (B,Q,3), flags=[bool]).  The projections are built so that most reference points land strictly inside
    the map: a plain view (u = W (a c + 1/2)-like rows, w = 1), a transformed view (T a rigid motion, P scaled for (r, phi deg,
    rho deg)), a perspective view (w = x); the clamped case overshoots the unit square by a tenth on every side."""
    g = torch.Generator().manual_seed(3000 + c.seed)
    B, Q, V = c.B, c.Q, n_views(c)
    lo, hi = (-0.1, 1.1) if c.special == "clamped" else (0.12, 0.88)
    center0 = torch.stack([a + (b - a) * torch.rand(B, Q, generator=g) for a, b in BOX], -1)
    if c.special == "wzero":
        center0[..., 2] = (torch.arange(Q) % 3).float()           # z = 0 for every third query: w = z there
    views, shape, projection, flags = [], [], [], []
    for v in range(V):
        L = c.LP[v][0]
        views.append(OrderedDict((str(l), torch.randn(B, LEVELS[l][0], LEVELS[l][1], 16, generator=g)) for l in range(L)))
        H, W = IMAGES[v]
        shape.append(torch.tensor([[H, W]] * B, dtype=torch.int64))
        T = torch.zeros(B, 4, 4)
        P = torch.zeros(B, 3, 4)
        kind = "wzero" if c.special == "wzero" else KINDS[v]
        for b in range(B):
            sh = 0.01 * b                                           # every batch element its own matrices
            if kind == "plain":
                ax, ay = (0, 1) if v == 0 else (1, 2)               # the second plain view looks along another axis pair
                gu, ou = _affine(*BOX[ax], lo + sh, hi)
                gv, ov = _affine(*BOX[ay], lo, hi - sh)
                P[b, 0, ax], P[b, 0, 3] = W * gu, W * ou
                P[b, 1, ay], P[b, 1, 3] = H * gv, H * ov
                P[b, 2, 3] = 1.0
            elif kind == "transformed":
                a = 0.1 + 0.05 * b                                  # a turn about z and a shift
                T[b] = torch.tensor([[math.cos(a), -math.sin(a), 0.0, 1.0 + b], [math.sin(a), math.cos(a), 0.0, -0.5],
                                     [0.0, 0.0, 1.0, 0.3], [0.0, 0.0, 0.0, 1.0]])
                gu, ou = _affine(0.0, 70.0, lo, hi)                 # r
                gv, ov = _affine(-80.0, 80.0, lo, hi)               # phi in degrees
                P[b, 0, 0], P[b, 0, 3] = W * gu, W * ou
                P[b, 1, 1], P[b, 1, 3] = H * gv, H * ov
                P[b, 1, 2] = H * 0.002                              # a little rho
                P[b, 2, 3] = 1.0
            elif kind == "perspective":
                P[b, 0, 0], P[b, 0, 1] = W * 0.5, W * (0.13 + sh)   # u = W (1/2 + 0.13 y / x)
                P[b, 1, 0], P[b, 1, 2] = H * 0.4, H * 0.5           # v = H (0.4 + 0.5 z / x)
                P[b, 2, 0] = 1.0
            else:                                                   # wzero: row 2 = (0, 0, 1, 0) as in kradar's query grid
                gu, ou = _affine(*BOX[0], 0.2, 0.9)
                gv, ov = _affine(*BOX[1], 0.2, 0.9)
                P[b, 0, 0], P[b, 0, 3] = W * gu, W * ou
                P[b, 1, 1], P[b, 1, 3] = H * gv, H * ov
                P[b, 2, 2] = 1.0
        projection.append((T, P))
        flags.append(kind == "transformed")
    return dict(views=views, shape=shape, projection=projection, center0=center0, flags=flags)


def form_inputs(inp, form):
    """The forms case: the same values in another form -> (shape list, projection list, has_transformation)."""
    shape, projection, flags = list(inp["shape"]), list(inp["projection"]), None
    if form == "flags":
        flags = list(inp["flags"])
    elif form == "p4":
        row = torch.tensor([0.0, 0.0, 0.0, 1.0])
        projection = [(T, torch.cat((P, row.expand(P.shape[0], 1, 4)), 1)) for T, P in projection]
    elif form == "shape-stride3":
        shape = [torch.cat((s, torch.full((s.shape[0], 1), 3, dtype=torch.int64)), 1) for s in shape]      # (B,3) rows
    elif form == "shape-int32":
        shape = [s.to(torch.int32) for s in shape]
    else:
        assert form == "none", form
    return shape, projection, flags


# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------
@contextmanager
def _recorded(trace):
    """Record what the oracle computes on the way: the reference points of every (iteration, view) and the sampling locations of
    every (iteration, view) with the level sizes."""
    from oracle import dprt_oracle as O
    ref_points, deform = O.reference_points, O.ms_deform_attn

    def rp(*a, **k):
        r = ref_points(*a, **k)
        trace["refs"].append(r.detach())
        return r

    def da(*a, **k):
        def core(value, shapes, loc, aw):
            trace["locs"].append((list(shapes), loc.detach()))
            return O.msda_core(value, shapes, loc, aw)
        return deform(*a, core=core, **k)
    O.reference_points, O.ms_deform_attn = rp, da
    try:
        yield
    finally:
        O.reference_points, O.ms_deform_attn = ref_points, deform


def reference(c, fuser, inp, dtype=torch.float64):
    """-> (out, trace): the oracle's IMPFusion in ``dtype`` on the CPU with "center" replaced by center - center0; trace["refs"]
    [it * V + v] (B,Q,2), trace["locs"][it * V + v] = ([(H, W)], (B,Q,8,L,P,2))."""
    from oracle import dprt_oracle as O
    cast = lambda t: t.to(dtype) if t.is_floating_point() else t
    views = [[cast(l) for l in lv.values()] for lv in inp["views"]]
    proj = [(cast(T), cast(P)) for T, P in inp["projection"]]
    shapes = [s.to(dtype) for s in inp["shape"]]
    trace = {"refs": [], "locs": []}
    with torch.no_grad(), _recorded(trace):
        out = O.impfusion(views, shapes, proj, cast(inp["center0"]), state_dict64(fuser, dtype), "f", oracle_cfg(c))
    out = OrderedDict((k, v) for k, v in out.items())
    out["center"] = out["center"] - cast(inp["center0"])
    return out, trace


_CACHE = {}


def cached(c):
    """(fuser on the CPU, inputs, fp64 out, trace, fp32 out, fp64 attn0, fp32 attn0) of a case, computed once per process and
    left unchanged."""
    if c.name not in _CACHE:
        fuser, inp = make_fuser(c), make_inputs(c)
        out64, trace = reference(c, fuser, inp)
        out32, _ = reference(c, fuser, inp, torch.float32)
        _CACHE[c.name] = (fuser, inp, out64, trace, out32, attn0_reference(fuser), attn0_reference(fuser, torch.float32))
    return _CACHE[c.name]


def qk_rows(fuser, it=0, x=None, dtype=torch.float64):
    """q, k rows of layer ``it`` in the kernel's exp2 domain: (V,8,Q,2) each, q pre-scaled by log2(e) / sqrt(2); input
    ``x`` (Q,16) defaults to the learned query table."""
    x = (fuser.query if x is None else x).detach().to(dtype)
    qk = x + fuser.query_embedding.weight.detach().to(dtype)
    qs, ks = [], []
    for ml in fuser.mpfusion[f"fusion{it}"].ml_fusion_layers.values():
        w, b = ml.self_attn.in_proj_weight.detach().to(dtype), ml.self_attn.in_proj_bias.detach().to(dtype)
        qs.append((qk @ w[:16].T + b[:16]).view(-1, 8, 2).transpose(0, 1) * (math.log2(math.e) / math.sqrt(2.0)))
        ks.append((qk @ w[16:32].T + b[16:32]).view(-1, 8, 2).transpose(0, 1))
    return torch.stack(qs), torch.stack(ks)


def attn0_reference(fuser, dtype=torch.float64):
    """First-layer attention output before out_proj, (V,Q,16): softmax(q k^T / sqrt(2)) v per head, q and k from query +
    query_embedding, v from query -- what dpft_decoder_attn0_f32 makes from the weights."""
    x = fuser.query.detach().to(dtype)
    qk = x + fuser.query_embedding.weight.detach().to(dtype)
    outs = []
    for ml in fuser.mpfusion["fusion0"].ml_fusion_layers.values():
        w, b = ml.self_attn.in_proj_weight.detach().to(dtype), ml.self_attn.in_proj_bias.detach().to(dtype)
        q = (qk @ w[:16].T + b[:16]).view(-1, 8, 2).transpose(0, 1)
        k = (qk @ w[16:32].T + b[16:32]).view(-1, 8, 2).transpose(0, 1)
        v = (x @ w[32:].T + b[32:]).view(-1, 8, 2).transpose(0, 1)
        att = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(2.0), -1)
        outs.append((att @ v).transpose(0, 1).reshape(-1, 16))
    return torch.stack(outs)


def slice_log2_den(q, k, NS):
    """log2 of the one-pass denominator sum_k exp2(q.k - |q| max_slice |k|) per (..., query, slice): the kernel redoes a slice
    whose value is below -100.  q, k (...,Q,2) in the exp2 domain."""
    Q = k.shape[-2]
    SL = -(-Q // NS)
    s = q @ k.transpose(-1, -2)
    out = torch.full(s.shape[:-1] + (NS,), float("nan"), dtype=s.dtype)
    for sl in range(NS):
        k0, k1 = sl * SL, min(Q, (sl + 1) * SL)
        if k1 <= k0:
            continue
        ref = q.norm(dim=-1, keepdim=True) * k[..., k0:k1, :].norm(dim=-1).amax(-1)[..., None, None]
        out[..., sl] = torch.logsumexp((s[..., k0:k1] - ref) * math.log(2.0), -1) / math.log(2.0)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------
def tolerance(ref):
    """Elementwise bound rtol |ref| + atol with atol = 1e-5 max|ref|."""
    ref = ref.detach().double().cpu()
    return RTOL * ref.abs() + ATOL_SCALE * max(float(ref.abs().max()), 1e-6)


def distance(a, ref):
    """max |a - ref| / tolerance(ref): at most 1 passes the fixed rule."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float(((a - ref).abs() / tolerance(ref)).max())


def argmax_rows(ref_cls):
    """Rows whose fp64 top-2 margin exceeds ten times the absolute tolerance: (B,Q) bool.  One class: every row."""
    ref_cls = ref_cls.double()
    if ref_cls.shape[-1] < 2:
        return torch.ones(ref_cls.shape[:-1], dtype=torch.bool)
    top = ref_cls.topk(2, -1).values
    return (top[..., 0] - top[..., 1]) > 10 * ATOL_SCALE * float(ref_cls.abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# the input conditions, on the fp64 reference alone
# ---------------------------------------------------------------------------------------------------------------------
def check_inputs(c, out64, trace):
    """-> dict of figures; raises AssertionError when the case's inputs would let an error hide."""
    V = n_views(c)
    fig = {}
    assert len(trace["refs"]) == len(trace["locs"]) == c.iters * V
    at0 = at1 = 0
    for i, r in enumerate(trace["refs"]):
        inside = ((r > 0) & (r < 1)).all(-1).double().mean()
        assert inside >= 0.5, (c.name, "iteration", i // V, "view", i % V, "reference points strictly inside", float(inside))
        at0 += int((r == 0).sum())
        at1 += int((r == 1).sum())
    fig["refs_at_0"], fig["refs_at_1"] = at0, at1
    if c.special == "clamped":
        assert at0 >= 1 and at1 >= 1, (c.name, at0, at1)
    n_in = n_all = 0
    near = float("inf")
    for i, (shapes, loc) in enumerate(trace["locs"]):
        for l, (H, W) in enumerate(shapes):
            tx, ty = loc[:, :, :, l, :, 0] * W - 0.5, loc[:, :, :, l, :, 1] * H - 0.5
            ok = (tx > -1) & (tx < W) & (ty > -1) & (ty < H)
            assert int(ok.sum()) >= 1, (c.name, "iteration", i // V, "view", i % V, "level", l, "no in-map sample")
            n_in += int(ok.sum())
            n_all += ok.numel()
            near = min(near, float((tx + 1).abs().min()), float((ty + 1).abs().min()))
    fig["in_map"] = n_in / n_all
    assert fig["in_map"] >= 0.5, (c.name, fig["in_map"])
    fig["nearest_to_minus_1"] = near
    assert near > 1e-6, (c.name, near)       # the one point where grid_sample and the floor rule differ (tests/test_sampler_rule.py)
    for k in KEYS:
        fig["max_" + k] = float(out64[k].abs().max())
        assert fig["max_" + k] >= 0.1, (c.name, k, fig["max_" + k])
    rows = argmax_rows(out64["class"])
    fig["argmax_exempt"] = 1.0 - float(rows.double().mean())
    assert fig["argmax_exempt"] <= 0.05, (c.name, fig["argmax_exempt"])
    return fig


def table_rows():
    rows = []
    for c in CASES:
        lp = ",".join(f"{l}/{p}" for l, p in c.LP)
        rows.append(f"{c.name:15s} B={c.B} Q={c.Q:4d} V={n_views(c)} L/P {lp:19s} iters={c.iters} ncls={c.ncls:2d}  {c.why}")
    return rows


if __name__ == "__main__":
    print("\n".join(table_rows()))
