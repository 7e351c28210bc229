"""TEST INFRASTRUCTURE -- the lattice of tests/test_xattn_lattice.py (CPU) and tests/test_gpu_xattn_lattice.py (GPU).

The TRAINING decoder's deformable cross-attention + FFN block (dpft_amd/csrc/decoder_train_x.hip: xf_train_fwd_kernel,
xf_train_bwd_kernel<SAVED>, xf_scatter_small_kernel, through train_fused.xattn_ffn_blocks and the two C entries) in front of the
fp64 oracle -- O.ms_deform_attn with the floor core, O._ln, F.linear / F.mish / F.linear, O._ln, autograd for every gradient --
at the shapes where such a block goes wrong (the numbers are the items of ``ITEMS``):

   1  V = 4 (the dropout element index runs across views)              6  scatter chunking: Q below the chunk count, a last
   2  views with different (L, P) in one launch                           chunk of one row, fewer than 8 chunks
   3  L = 8: eight small maps in a view, more than the five record     7  the 2048-pixel limit recorded / atomics, the 256-pixel
      slots, with a tie in the pixel-count order at the cut               limit replicated / plain, both kinds in one call
   4  saved == NULL: the backward that gathers again                   8  dy1, d pos and all 16 parameter gradients, the dqp
   5  row blocks that straddle batch elements, Q = 1, B Q that            route through a non-zero sampling_offsets.weight
      wraps the 32 replicas twice                                      9  saturated Mish, a flat LayerNorm2 row, logits 120
  10  the entries' refusals (tests/test_xattn_lattice.py)                 apart, a view whose every sample is outside

No kinks, by construction: d ref and d offsets are piecewise smooth, and an fp32 rounding that changed the bilinear cell would
change the slope.  Every row's reference point is drawn from the case's generator and REDRAWN until each of its L P 8 sample
positions t = loc * size - 0.5 (fp64, from the case's real weights) is at least 2^-10 pixel away from every integer in [-1, size],
and a float32 replay of the positions stays within 2^-10 / 64 of them.  No row is ever left out.  fp32 spaces its numbers 2^-16
apart from 128 on, so on an axis longer than 128 pixels the reference points keep to the part where the positions stay below that.

Gates, both the project's own: the forward under tests.decoder_lattice.tolerance (1e-4 |ref| + 1e-5 max|ref|, element-wise), every
gradient under grad_close of tests/test_gpu_sampler_edges.py (atol = max(4 x max|fp32 oracle - fp64|, 1e-5 max|ref|), 1e-4
relative, element-wise).  ``gate_ratio`` restates the second only to print |got - fp64| over the gate.

No GPU code here.  ``python -m tests.xattn_lattice`` prints the table."""
from collections import namedtuple

import torch
import torch.nn.functional as F

from tests.decoder_lattice import distance, tolerance  # noqa: F401  (the forward rule)

A = "ms_deform_attn."
PARAMS = [A + "sampling_offsets.weight", A + "sampling_offsets.bias", A + "attention_weights.weight", A + "attention_weights.bias",
          A + "value_proj.weight", A + "value_proj.bias", A + "output_proj.weight", A + "output_proj.bias", "norm2.weight",
          "norm2.bias", "ffn1.weight", "ffn1.bias", "ffn2.weight", "ffn2.bias", "norm3.weight", "norm3.bias"]      # = view_params()[6:]
KINK = 2.0 ** -10                 # every position is at least this far from an integer in [-1, size]
REPLAY = KINK / 64                # and its float32 replay at most this far from it
LONG, LONG_KEEP = 128, 96         # an axis longer than LONG: ref * size stays below LONG_KEEP
MAX_SLOTS, REC_PIXELS, TINY_PIXELS, REPLICAS, NUM_CU = 5, 2048, 256, 32, 256      # decoder_train_x.hip / PyramidState / host_consts.h
MISH_PLACED = (100.0, -100.0, 60.0, -60.0, 25.0, -25.0, 20.5, -20.5, 20.0, -20.0, 19.5, -19.5, 1.0, -1.0, 0.0,
               89.0, -89.0, 104.0, -104.0,          # expf overflows from 88.73 on: exp(x) in the softplus, exp(-x) in the sigmoid
               40.0, -40.0, 15.0, -15.0, 10.0, -10.0, 5.0, -5.0, 3.0, -3.0, 0.5, -0.5, 2.0)
PYR5 = ((13, 9), (7, 5), (4, 3), (2, 2), (1, 1))

Case = namedtuple("Case", "name B Q lp maps p_drop seeds salt special seed why")

CASES = [
    Case("v4-mixed", 3, 7, ((5, 4), (1, 1), (8, 2), (3, 3)),
         (((40, 64), (20, 32), (10, 16), (5, 8), (3, 4)), ((7, 5),),
          ((4, 6), (16, 20), (6, 4), (2, 3), (3, 8), (1, 5), (10, 12), (2, 2)), ((12, 9), (6, 5), (1, 1))), 0.0, (0,), 1, "", 1000,
         "items 1-5, 8: V = 4; L P = 20 beside 1; 21 rows = 1 mod 4, blocks straddle b at rows 7 and 14; L = 8: eight small maps, "
         "4x6 6x4 3x8 of 24 pixels each with the cut of five slots between them, so 5 recorded and 3 on atomics"),
    Case("one-row", 1, 1, ((2, 4),), (((9, 13), (4, 3)),), 0.0, (0,), 1, "", 2000,
         "items 5, 6: one live wave of four; the scatter with Q = 1 below its 8 chunks"),
    Case("q1-b2", 2, 1, ((1, 4), (4, 1)), (((11, 6),), ((8, 8), (5, 7), (3, 2), (1, 1))), 0.0, (0,), 1, "", 3000,
         "items 2, 5: Q = 1 with B = 2: every row another batch element; P = 4 beside P = 1"),
    Case("wrap-replicas", 5, 13, ((3, 2), (2, 3)), (((16, 16), (257, 1), (1, 1)), ((1, 40), (9, 7))), 0.0, (0,), 1, "", 4000,
         "items 2, 4, 5, 7: 65 rows: bq % 32 wraps twice; 16x16 = 256 pixels (replicated) beside 257x1 (plain); Hx1, 1xW, 1x1 maps"),
    Case("limit-2048", 2, 9, ((3, 4),), (((32, 64), (3, 683), (8, 8)),), 0.0, (0,), 1, "", 5000,
         "items 6, 7: 32x64 = 2048 pixels (recorded) beside 3x683 = 2049 (atomics); qchunk 2, the last chunk one row"),
    Case("chunks-4", 4, 7, ((4, 2),) * 4, tuple(((12 + v, 9), (6, 5 + v), (3, 4), (2, 2 + v)) for v in range(4)), 0.0, (0,), 1, "", 6000,
         "items 1, 6: four small maps a view, n_maps B = 64, so 4 chunks (below the cap of 8), the last of one row"),
    Case("dropout-v4", 2, 5, ((2, 2),) * 4, tuple(((10 + v, 7), (4, 5)) for v in range(4)), 0.25, (0x123456789ABCDEF1, -5), 9, "", 7000,
         "items 1, 4: p = 0.25 at V = 4, the element index vbq * 16 + c across views; a seed with bits above 2^32 and a negative "
         "one; salt 9; masks replayed"),
    Case("dropout-odd", 1, 3, ((5, 4),), (PYR5,), 0.5, (3,), 1, "", 8000, "p = 0.5 at L P = 20, three rows"),
    Case("mish-sat", 2, 8, ((2, 2),), (((9, 12), (4, 5)),), 0.0, (0,), 1, "mish-sat", 9000,
         "item 9: ffn1.bias at +-100, +-60, +-25, +-20.5, +-20, +-19.5 (the x > 20 switch), +-89, +-104 (expf overflows), ...; "
         "ffn1.weight / 64 keeps the pre-activation within 0.1 of the placed value"),
    Case("flat-ln2", 2, 4, ((2, 2), (2, 2)), (((9, 12), (4, 5)),) * 2, 0.0, (0,), 1, "flat-ln2", 10000,
         "item 9: view 1 has output_proj = 0 and constant y1 rows on a 2^-6 grid: LayerNorm2 on a variance of exactly 0"),
    Case("void-view", 2, 6, ((3, 4), (3, 4)), (((20, 32), (10, 16), (5, 8)),) * 2, 0.0, (0,), 1, "void-view", 11000,
         "item 9: view 1 has sampling_offsets.weight = 0 and a bias of +64 pixels in x on maps up to 32 wide: every sample "
         "outside, mass 0, d refs and the maps' gradients exactly 0"),
    Case("softmax-120", 1, 6, ((5, 4),), (PYR5,), 0.0, (0,), 1, "softmax-120", 12000,
         "item 9: attention_weights.bias alternates +-60: logits 120 apart"),
]
# test_replicated_and_recorded_maps_in_one_call: (view, level) -> gradient replicas of the direct call
REPLICATED = Case("rep-and-rec", 2, 9, ((3, 2),), (((4, 4), (8, 8), (50, 50)),), 0.0, (0,), 1, "", 13000,
                  "item 7: a 4x4 map with 3 gradient replicas (atomics, bq % 3), a plain 8x8 map (recorded) and a 50x50 map "
                  "(atomics) in one call with a record buffer")
REPLICATED_REPS = {(0, 0): 3}
NOSAVE = ("v4-mixed", "wrap-replicas", "dropout-v4")       # test_backward_without_saved_features
RUNS = [(c, i) for c in CASES for i in range(len(c.seeds))]


def by_name(name):
    return next(c for c in CASES + [REPLICATED] if c.name == name)


def run_id(run):
    c, i = run
    return c.name if len(c.seeds) == 1 else f"{c.name}-seed{i}"


def n_views(c):
    return len(c.lp)


def items_of(c):
    """The items that the head of a case's ``why`` names ("items 1-5, 8: ...")."""
    head = c.why.split(":")[0]
    if not head.startswith("item"):
        return set()
    out = set()
    for part in head.split(" ", 1)[1].split(","):
        lo, _, hi = part.strip().partition("-")
        out |= set(range(int(lo), int(hi or lo) + 1))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the host side of dpft_xattn_ffn_train_bwd_f32 and of XattnFfnBlocksFn.backward, restated
# ---------------------------------------------------------------------------------------------------------------------
def scatter_plan(c, reps=None):
    """With a record buffer: slot of every (view, level) (-1 = atomics), the number of recorded maps, the chunk count before
    and after the cap and the rounding, and the rows of a chunk.  ``reps``: {(view, level): gradient replicas > 1}; the
    autograd Function passes plain buffers (XF_SCATTER = True), so none."""
    reps = reps or {}
    slots, n_maps = [], 0
    for v, maps in enumerate(c.maps):
        px = [h * w for h, w in maps]
        order = sorted((l for l in range(len(maps)) if px[l] <= REC_PIXELS and reps.get((v, l), 1) == 1), key=lambda l: px[l])
        slot = [-1] * len(maps)
        for i, l in enumerate(order[:MAX_SLOTS]):                  # sorted() is stable, as the insertion sort of the entry
            slot[l] = i
        n_maps += min(len(order), MAX_SLOTS)
        slots.append(slot)
    if not n_maps:
        return dict(slots=slots, n_maps=0, nchunk0=0, nchunk=0, qchunk=0, last=0)
    nchunk0 = min(8, max(1, NUM_CU // (n_maps * c.B)))
    qchunk = -(-c.Q // nchunk0)
    nchunk = -(-c.Q // qchunk)
    return dict(slots=slots, n_maps=n_maps, nchunk0=nchunk0, nchunk=nchunk, qchunk=qchunk, last=c.Q - (nchunk - 1) * qchunk)


def replicated_levels(c):
    """XF_SCATTER = False: the (view, level) maps that PyramidState replicates 32 times."""
    return [(v, l) for v, maps in enumerate(c.maps) for l, (h, w) in enumerate(maps) if h * w <= TINY_PIXELS]


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _sizes(maps, dtype):
    return torch.tensor([[w, h] for h, w in maps], dtype=dtype)          # (L, 2) ordered (x, y)


def positions(ref, off, maps):
    """t = loc * size - 0.5 in the dtype of ``ref``: ref (..., 2), off (..., 8, L, P, 2) -> (..., 8, L, P, 2), the kernels' order
    of operations (loc = ref + off / size)."""
    size = _sizes(maps, ref.dtype)[:, None, :]
    loc = ref[..., None, None, None, :] + off / size
    return loc * size - 0.5


def offsets(y1v, pos, p, L, P):
    qp = y1v + pos.unsqueeze(0)
    off = F.linear(qp, p[A + "sampling_offsets.weight"].to(qp.dtype), p[A + "sampling_offsets.bias"].to(qp.dtype))
    return off.view(*qp.shape[:-1], 8, L, P, 2)


def _near_kink(t, maps):
    size = _sizes(maps, t.dtype)[:, None, :]
    n = torch.round(t)
    return (n >= -1) & (n <= size) & ((t - n).abs() < KINK)


def inside(t, maps):
    size = _sizes(maps, t.dtype)[:, None, :]
    return ((t > -1) & (t < size)).all(-1)


def make_inputs(c, seed=None):
    """fp32 CPU inputs of a case: y1 (V,B,Q,16), pos (Q,16), refs (V,B,Q,2), the cotangent gy, per view the 16 parameters (a
    dict in PARAMS order) and the maps (B,H,W,16); ``redraws``: how often a row's reference point was drawn again."""
    seed = c.seed if seed is None else seed
    g = torch.Generator().manual_seed(seed)
    V, B, Q = n_views(c), c.B, c.Q
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    y1 = (randn(V, B, Q, 16) * 0.7).float()
    pos = (randn(Q, 16) * 0.5).float()
    gy = randn(V, B, Q, 16).float()
    params, feats = [], []
    for v, ((L, P), maps) in enumerate(zip(c.lp, c.maps)):
        assert len(maps) == L
        n = 8 * L * P
        # 0.08 of the map (of 64 pixels on a longer axis) and the weight's ~1 pixel: about a tenth of the samples outside
        bias = randn(8, L, P, 2) * 0.08 * _sizes(maps, torch.float64).clamp(max=64.0)[None, :, None, :]
        p = {A + "sampling_offsets.weight": randn(2 * n, 16) * 0.3,
             A + "sampling_offsets.bias": bias.reshape(-1),
             A + "attention_weights.weight": randn(n, 16) * 0.3, A + "attention_weights.bias": randn(n) * 0.5,
             A + "value_proj.weight": randn(16, 16) * 0.3, A + "value_proj.bias": randn(16) * 0.3,
             A + "output_proj.weight": randn(16, 16) * 0.3, A + "output_proj.bias": randn(16) * 0.2,
             "norm2.weight": 1 + randn(16) * 0.2, "norm2.bias": randn(16) * 0.2,
             "ffn1.weight": randn(32, 16) * 0.25, "ffn1.bias": randn(32) * 0.3,
             "ffn2.weight": randn(16, 32) * 0.2, "ffn2.bias": randn(16) * 0.2,
             "norm3.weight": 1 + randn(16) * 0.2, "norm3.bias": randn(16) * 0.2}
        assert list(p) == PARAMS
        if c.special == "mish-sat":
            p["ffn1.bias"] = torch.tensor(MISH_PLACED, dtype=torch.float64)
            p["ffn1.weight"] = p["ffn1.weight"] / 64
        if c.special == "softmax-120":
            p[A + "attention_weights.bias"] = 60.0 * (1 - 2 * (torch.arange(n, dtype=torch.float64) % 2))
        if c.special == "flat-ln2" and v == 1:
            p[A + "output_proj.weight"] = torch.zeros(16, 16, dtype=torch.float64)
            p[A + "output_proj.bias"] = torch.zeros(16, dtype=torch.float64)
            y1[v] = (torch.round(randn(B, Q, 1) * 0.7 * 64) / 64).float().expand(B, Q, 16)
        if c.special == "void-view" and v == 1:
            p[A + "sampling_offsets.weight"] = torch.zeros(2 * n, 16, dtype=torch.float64)
            bias[..., 0] = 64.0
            p[A + "sampling_offsets.bias"] = bias.reshape(-1)
        params.append({k: t.float() for k, t in p.items()})
        feats.append([(randn(B, h, w, 16) * 0.8).float() for h, w in maps])
    # reference points, row by row, redrawn until no position is near a kink and the float32 replay agrees
    refs = torch.zeros(V, B, Q, 2)
    redraws = 0
    for v, ((L, P), maps) in enumerate(zip(c.lp, c.maps)):
        span = torch.tensor([min(1.0, LONG_KEEP / s) if s > LONG else 1.0 for s in (max(w for _, w in maps), max(h for h, _ in maps))],
                            dtype=torch.float64)
        off64 = offsets(y1[v].double(), pos.double(), params[v], L, P)
        off32 = offsets(y1[v], pos, params[v], L, P)
        for b in range(B):
            for q in range(Q):
                for _ in range(1000):
                    r32 = (torch.rand(2, generator=g, dtype=torch.float64) * span).float()
                    t64 = positions(r32.double(), off64[b, q], maps)
                    t32 = positions(r32, off32[b, q], maps).double()
                    if (not _near_kink(t64, maps).any() and float((t32 - t64).abs().max()) <= REPLAY
                            and torch.equal(torch.floor(t32), torch.floor(t64))):
                        break
                    redraws += 1
                else:
                    raise AssertionError((c.name, v, b, q, "no reference point without a kink"))
                refs[v, b, q] = r32
    return dict(y1=y1, pos=pos, refs=refs, gy=gy, params=params, feats=feats, redraws=redraws)


# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------
def grad_names(c):
    return (["y1", "pos", "refs"] + [f"v{v}.map{l}" for v, maps in enumerate(c.maps) for l in range(len(maps))]
            + [f"v{v}.{n}" for v in range(n_views(c)) for n in PARAMS])


def tensor_class(name):
    """The classes of the figures in DESIGN.md."""
    if name in ("y3", "y1", "pos", "refs"):
        return name if name == "y3" else "d " + name
    tail = name.split(".", 1)[1]
    return "d maps" if tail.startswith("map") else ("d MSDeformAttn parameters" if tail in PARAMS[:6] else "d other parameters")


def block(P, y1v, pos, refv, levels, sd, masks=None):
    """One view: y3 = LN3(y2 + d4 ffn2(d3 Mish(ffn1(y2)))), y2 = LN2(y1 + d2 MSDeformAttn(y1 + pos, ref, levels))."""
    from oracle import dprt_oracle as O
    d2, d3, d4 = masks if masks is not None else (1.0, 1.0, 1.0)
    ca = O.ms_deform_attn(y1v + pos.unsqueeze(0), refv, levels, sd, "ml.ms_deform_attn", 8, P, core=O.msda_core_floor)
    y2 = O._ln(y1v + ca * d2, sd, "ml.norm2")
    hid = F.mish(F.linear(y2, sd["ml.ffn1.weight"], sd["ml.ffn1.bias"])) * d3
    ff = F.linear(hid, sd["ml.ffn2.weight"], sd["ml.ffn2.bias"])
    return O._ln(y2 + ff * d4, sd, "ml.norm3")


def masks_of(c, si, dtype):
    if c.p_drop == 0:
        return None
    from tests.dropout_masks import xattn_ffn_masks
    return [torch.from_numpy(m).to(dtype) for m in xattn_ffn_masks(c.seeds[si], c.salt, c.p_drop, n_views(c), c.B, c.Q)]


def reference(c, inp, dtype=torch.float64, si=0):
    """The oracle in ``dtype`` on the CPU with autograd -> dict(y3, grads {name: tensor} in grad_names order)."""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)   # noqa: E731
    y1, pos, refs = leaf(inp["y1"]), leaf(inp["pos"]), leaf(inp["refs"])
    feats = [[leaf(t) for t in fv] for fv in inp["feats"]]
    sds = [{"ml." + k: leaf(t) for k, t in p.items()} for p in inp["params"]]
    m = masks_of(c, si, dtype)
    outs = [block(c.lp[v][1], y1[v], pos, refs[v], feats[v], sds[v], None if m is None else [x[v] for x in m])
            for v in range(n_views(c))]
    out = torch.stack(outs)
    leaves = [y1, pos, refs] + [t for fv in feats for t in fv] + [sd["ml." + n] for sd in sds for n in PARAMS]
    grads = torch.autograd.grad(out, leaves, inp["gy"].to(dtype))
    return dict(y3=out.detach(), grads=dict(zip(grad_names(c), [t.detach() for t in grads])))


_CACHE, _REFS = {}, {}


def cached(c):
    if c.name not in _CACHE:
        _CACHE[c.name] = make_inputs(c)
    return _CACHE[c.name]


def cached_reference(c, dtype=torch.float64, si=0):
    """``reference`` once per (case, dtype, dropout seed) and left unchanged."""
    key = (c.name, dtype, si)
    if key not in _REFS:
        _REFS[key] = reference(c, cached(c), dtype, si)
    return _REFS[key]


def gate_ratio(got, ref64, ref32):
    """max |got - fp64| / (atol + 1e-4 |fp64|) with grad_close's atol = max(4 max|fp32 - fp64|, 1e-5 max|fp64|): at most 1 passes."""
    got, ref64, ref32 = (t.detach().double().cpu() for t in (got, ref64, ref32))
    atol = max(4 * float((ref32 - ref64).abs().max()), 1e-5 * max(float(ref64.abs().max()), 1e-6))
    return float(((got - ref64).abs() / (atol + 1e-4 * ref64.abs())).max())


def expected_zero(c):
    """Gradients that are identically zero by the case's construction."""
    # a softmax over one sample is constant
    zero = {f"v{v}.{n}" for v, (l, p) in enumerate(c.lp) if l * p == 1 for n in PARAMS[2:4]}
    if c.special == "flat-ln2":        # nothing flows through a zero output_proj
        zero |= {f"v1.map{l}" for l in range(c.lp[1][0])} | {"v1." + n for n in PARAMS[:6]}
    if c.special == "void-view":       # no sample inside: only output_proj.bias sees the attention's gradient
        zero |= {f"v1.map{l}" for l in range(c.lp[1][0])} | {"v1." + n for n in PARAMS[:7]}
    return zero


def expected_exact(c):
    """Non-zero gradients that float32 gives exactly: with one row a view, d norm3.bias is the cotangent itself."""
    return {f"v{v}.norm3.bias" for v in range(n_views(c))} if c.B * c.Q == 1 else set()


# ---------------------------------------------------------------------------------------------------------------------
# the input conditions
# ---------------------------------------------------------------------------------------------------------------------
def check_inputs(c, inp=None):
    """-> dict of figures; raises AssertionError where a case's inputs are not what the case says."""
    inp = cached(c) if inp is None else inp
    fig = dict(rows=n_views(c) * c.B * c.Q, rows_dropped=0, redraws=inp["redraws"])
    n_in = n_all = 0
    per_view = []
    for v, ((L, P), maps) in enumerate(zip(c.lp, c.maps)):
        t64 = positions(inp["refs"][v].double(), offsets(inp["y1"][v].double(), inp["pos"].double(), inp["params"][v], L, P), maps)
        t32 = positions(inp["refs"][v], offsets(inp["y1"][v], inp["pos"], inp["params"][v], L, P), maps).double()
        assert tuple(t64.shape) == (c.B, c.Q, 8, L, P, 2)
        assert not _near_kink(t64, maps).any(), (c.name, v, "a position within 2^-10 of an integer")
        replay = float((t32 - t64).abs().max())
        fig["replay"] = max(fig.get("replay", 0.0), replay)
        assert replay <= REPLAY, (c.name, v, replay)
        assert torch.equal(torch.floor(t32), torch.floor(t64)), (c.name, v, "the float32 replay changes a cell")
        assert torch.equal(inside(t32, maps), inside(t64, maps)), (c.name, v)
        ins = inside(t64, maps)
        per_view.append(float(ins.double().mean()))
        n_in, n_all = n_in + int(ins.sum()), n_all + ins.numel()
        assert all(float(t.abs().max()) > 0 for t in inp["params"][v].values()) or c.special in ("flat-ln2", "void-view"), (c.name, v)
    fig["inside"] = per_view
    fig["outside"] = 1 - n_in / n_all
    void = 1 if c.special == "void-view" else None
    for v, f in enumerate(per_view):
        assert (f == 0.0) if v == void else (0.0 < f < 1.0), (c.name, v, f, "samples in and out")
    return fig


def table_rows():
    rows = []
    for c in CASES + [REPLICATED]:
        lp = " ".join(f"({l},{p})" for l, p in c.lp)
        maps = " | ".join(" ".join(f"{h}x{w}" for h, w in m) for m in c.maps)
        drop = f" p={c.p_drop} seeds {c.seeds} salt {c.salt}" if c.p_drop else ""
        rows.append(f"{c.name:13s} B={c.B} Q={c.Q:2d} V={n_views(c)} (L,P) {lp}  maps {maps}{drop}: {c.why}")
    return rows


if __name__ == "__main__":
    print("\n".join(table_rows()))
    for case in CASES + [REPLICATED]:
        print(case.name, check_inputs(case))
