"""Every bilinear sampler of the project against ONE fp64 rule (oracle.dprt_oracle.msda_core_floor), element by element, on a
lattice that hits the border strips, the corners where two strips meet, exact pixel positions, t = -1, t = size, one-pixel maps
and +-2^20 pixels by construction (tests/sampler_lattice.py; tests/test_sampler_rule.py pins the rule itself on the CPU).

  1, 2  msda_fwd_kernel / msda_bwd_kernel          ops.msda_fwd / msda_bwd                 test_generic_operator_*
  3, 4  xattn_fwd_kernel / xattn_bwd_kernel        ops.xattn_fwd / xattn_bwd               test_xattn_operator_on_the_lattice
  5, 6  training block forward / backward          train_fused.xattn_ffn_blocks            test_training_block_on_the_lattice
        (per-corner atomics with replicas, and scatter records + xf_scatter_small_kernel)
  7     inference decoder                          model.fuser.use_fused_inference = True  test_inference_decoder_*

Tolerances.  Forward quantities and `mass`: the project's rule, rtol 1e-4, atol 1e-5 * max|ref|.  Gradients: the same
oracle run in float32 on the CPU on the same inputs gives, per tensor, its largest element-wise distance from the fp64 result;
the kernel is held to 4 x that distance (the kernels sum in another order -- wave reductions, atomics -- than torch's fp32 CPU
path), floored at the forward rule.  Nothing is calibrated on a kernel's own output.  Every figure is printed before it is
asserted (run with -s to see them)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import sampler_lattice as SL

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _worst(got, ref, atol, rtol):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    excess = (got - ref).abs() - (atol + rtol * ref.abs())
    i = int(excess.argmax())
    idx = tuple(int(v) for v in np.unravel_index(i, ref.shape)) if ref.dim() else ()
    return float(excess.max()), idx, float((got - ref).abs().max()), got, ref


def fwd_close(got, ref, what, where=None):
    """The project's forward rule, element-wise: rtol 1e-4, atol 1e-5 * max|ref|."""
    atol = 1e-5 * max(float(ref.abs().max()), 1e-6)
    excess, idx, err, got, ref = _worst(got, ref, atol, 1e-4)
    print(f"{what:44s} max|hip - fp64| {err:.3e}   gate atol {atol:.3e} + 1e-4 rel")
    assert excess <= 0, f"{what}: worst element {idx}: got {float(got[idx])!r} ref {float(ref[idx])!r}" + (where(idx) if where else "")


def grad_close(got, ref64, ref32, what, where=None):
    """4 x the fp32 CPU oracle's own largest element-wise distance from fp64 for this tensor, floored at the forward rule."""
    ref64 = ref64.detach().double()
    e32 = float((ref32.detach().double() - ref64).abs().max())
    atol = max(4 * e32, 1e-5 * max(float(ref64.abs().max()), 1e-6))
    excess, idx, err, got, ref = _worst(got, ref64, atol, 1e-4)
    print(f"{what:44s} max|hip - fp64| {err:.3e}   max|fp32 oracle - fp64| {e32:.3e}   gate atol {atol:.3e} + 1e-4 rel")
    assert excess <= 0, f"{what}: worst element {idx}: got {float(got[idx])!r} ref {float(ref[idx])!r}" + (where(idx) if where else "")


def _lsi(shapes):
    return [0] + [int(v) for v in np.cumsum([h * w for h, w in shapes])[:-1]]


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2: the generic operator
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("M,D", [(8, 2), (3, 5), (1, 1)])
@pytest.mark.parametrize("pyramid", ["pow2", "odd"])
def test_generic_operator_on_the_lattice(pyramid, M, D, P):
    """ops.msda_fwd / msda_bwd: out, grad_value, grad_loc, grad_attn.  "pow2": the full lattice, float32-exact (asserted);
    "odd": (13,9) (7,5) (3,7) with fractional parts .25 / .5 / .75 only -- no kinks, so rounding cannot change the cell
    (asserted) -- which keeps strides that are not powers of two covered."""
    from dpft_amd.hip import ops
    from oracle import dprt_oracle as O
    kinks = pyramid == "pow2"
    shapes = SL.POW2_SHAPES if kinks else SL.ODD_SHAPES
    t = SL.lattice_t(shapes, M, P, kinks)
    loc32 = SL.direct_loc(t, shapes)
    t32 = SL.replay_direct(loc32, shapes).astype(np.float64)
    assert np.isfinite(loc32).all() and np.abs(t).max() <= SL.FAR + 0.5
    if kinks:
        assert np.array_equal(t32, t), "the lattice is not exact in float32"            # cap on dropped points: 0
    else:
        assert np.array_equal(np.floor(t32), np.floor(t))
    SL.assert_coverage(t32, shapes, kinks, what=pyramid)
    g = torch.Generator().manual_seed(100 + 10 * M + P)
    L, Q, S = len(shapes), t.shape[0], sum(h * w for h, w in shapes)
    loc = torch.from_numpy(loc32)
    loc = torch.stack((loc, loc.roll(1, 0)))                                            # N = 2: the batch stride
    tt = np.stack((t32, np.roll(t32, 1, 0)))
    value = torch.randn(2, S, M, D, generator=g)
    attn = torch.rand(2, Q, M, L, P, generator=g) + 0.25
    go = torch.randn(2, Q, M * D, generator=g)

    def oracle(dt):
        v, l, a = (x.to(dt).requires_grad_(True) for x in (value, loc, attn))
        out = O.msda_core_floor(v, shapes, l, a)
        return (out.detach(),) + torch.autograd.grad(out, (v, l, a), go.to(dt))
    r64, r32 = oracle(torch.float64), oracle(torch.float32)
    sh_t = torch.tensor(shapes, dtype=torch.int64, device=DEV)
    lsi_t = torch.tensor(_lsi(shapes), dtype=torch.int64, device=DEV)
    args = (value.to(DEV), sh_t, lsi_t, loc.to(DEV), attn.to(DEV))
    out = ops.msda_fwd(*args)
    gv, gl, ga = ops.msda_bwd(*args, go.to(DEV))
    tag = f"msda {pyramid} M{M} D{D} P{P}"
    at = lambda idx: f" at t = {tt[idx[0], idx[1], idx[2], idx[3], idx[4]].tolist()} of level {shapes[idx[3]]}"
    fwd_close(out, r64[0], f"{tag} out")
    grad_close(gv, r64[1], r32[1], f"{tag} grad_value")
    grad_close(gl, r64[2], r32[2], f"{tag} grad_loc", at)
    grad_close(ga, r64[3], r32[3], f"{tag} grad_attn", at)
    if kinks:      # the rule on t == -1 / t == size: no slope at all (grid_sample would return the inside slope on t == -1)
        edge = torch.from_numpy((tt == -1) | (tt == SL.sizes_wh(shapes)[None, None, None, :, None, :]))
        assert edge.any() and (gl.cpu()[edge] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3, 4: fused sample-then-project operator
# ---------------------------------------------------------------------------------------------------------------------
def _xattn_oracle(core, dt, shapes, levels, ref, off, attn, Wv, bv, go, M, D):
    lv = [l.to(dt).requires_grad_(True) for l in levels]
    r, o, a, W, b = (x.to(dt).requires_grad_(True) for x in (ref, off, attn, Wv, bv))
    B = ref.shape[0]
    value = F.linear(torch.cat([l.flatten(1, 2) for l in lv], 1), W, b).view(B, -1, M, D)
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=dt)
    loc = r[:, :, None, None, None, :] + o / norm[None, None, None, :, None, :]
    out = core(value, shapes, loc, a)
    grads = torch.autograd.grad(out, [o, a, r, W, b] + lv, go.to(dt))
    with torch.no_grad():
        # the raw samples per head (before value_proj) and the in-bounds mass, from the same rule
        cat = torch.cat([l.flatten(1, 2) for l in lv], 1)                                # (B, S, C)
        samp = torch.stack([core(cat[:, :, None, :], shapes, loc[:, :, m:m + 1], a[:, :, m:m + 1]) for m in range(M)], 2)
        mass = core(torch.ones_like(cat[:, :, :1]).expand(-1, -1, M)[..., None].contiguous(), shapes, loc, a)
    return out.detach(), samp, mass, grads


@pytest.mark.parametrize("P", [1, 4])
def test_xattn_operator_on_the_lattice(P):
    """ops.xattn_fwd / xattn_bwd: out, samp, mass, goff, gattn, gref, every level gradient, and the value_proj gradients that
    the callers form from samp / mass.  `mass` also against its closed form: the sum of attention x in-bounds corner weights."""
    from dpft_amd.hip import ops
    from oracle import dprt_oracle as O
    shapes, M, D, C = SL.POW2_SHAPES, 8, 2, 16
    t = SL.lattice_t(shapes, M, P)
    ref32, off32 = SL.ref_off_split(t, shapes)
    assert np.isfinite(off32).all() and np.abs(off32).max() <= SL.FAR + 64
    assert np.array_equal(SL.replay_ref_off(ref32, off32, shapes).astype(np.float64), t), "the lattice is not exact in float32"
    SL.assert_coverage(t, shapes, what="xattn")
    g = torch.Generator().manual_seed(200 + P)
    L, Q, B = len(shapes), t.shape[0], 2
    ref = torch.from_numpy(ref32)
    off = torch.from_numpy(off32)
    ref, off = torch.stack((ref, ref.roll(7, 0))), torch.stack((off, off.roll(7, 0)))
    tt = np.stack((t, np.roll(t, 7, 0)))
    levels = [torch.randn(B, h, w, C, generator=g) for h, w in shapes]
    attn = torch.softmax(torch.randn(B, Q, M, L * P, generator=g), -1).view(B, Q, M, L, P)
    Wv, bv = torch.randn(C, C, generator=g) * 0.3, torch.randn(C, generator=g)
    go = torch.randn(B, Q, C, generator=g)
    r64 = _xattn_oracle(O.msda_core_floor, torch.float64, shapes, levels, ref, off, attn, Wv, bv, go, M, D)
    r32 = _xattn_oracle(O.msda_core_floor, torch.float32, shapes, levels, ref, off, attn, Wv, bv, go, M, D)
    # closed form of the mass, written out here: sum over (level, point) of attn x the bilinear weights of the corners in the map
    tq = torch.from_numpy(tt)
    wh = torch.from_numpy(SL.sizes_wh(shapes))[None, None, None, :, None, :]
    inside = ((tq > -1) & (tq < wh)).all(-1)
    lo = torch.floor(tq)
    fr = tq - lo
    wsum = torch.zeros(tq.shape[:-1], dtype=torch.float64)
    for dx in (0, 1):
        for dy in (0, 1):
            cx, cy = lo[..., 0] + dx, lo[..., 1] + dy
            ok = inside & (cx >= 0) & (cx <= wh[..., 0] - 1) & (cy >= 0) & (cy <= wh[..., 1] - 1)
            wgt = (fr[..., 0] if dx else 1 - fr[..., 0]) * (fr[..., 1] if dy else 1 - fr[..., 1])
            wsum += torch.where(ok, wgt, torch.zeros_like(wgt))
    mass_closed = (attn.double() * wsum).sum((-1, -2))
    torch.testing.assert_close(r64[2].view(B, Q, M), mass_closed, rtol=1e-12, atol=1e-12)
    lv_dev = [l.to(DEV) for l in levels]
    dev = [x.to(DEV) for x in (ref, off, attn, Wv, bv)]
    out, samp, mass = ops.xattn_fwd(lv_dev, *dev, M, P)
    grads = [torch.zeros_like(l) for l in lv_dev]
    goff, gattn, gref = ops.xattn_bwd(lv_dev, grads, *dev, go.to(DEV), M, P)
    tag = f"xattn P{P}"
    at = lambda idx: f" at t = {tt[idx[0], idx[1], idx[2], idx[3], idx[4]].tolist()} of level {shapes[idx[3]]}"
    fwd_close(out, r64[0], f"{tag} out")
    fwd_close(samp, r64[1].view(B, Q, M, C), f"{tag} samp")
    fwd_close(mass, mass_closed, f"{tag} mass (closed form)")
    g64, g32 = r64[3], r32[3]
    grad_close(goff, g64[0], g32[0], f"{tag} goff", at)
    grad_close(gattn, g64[1], g32[1], f"{tag} gattn", at)
    grad_close(gref, g64[2], g32[2], f"{tag} gref")
    g4 = go.to(DEV).view(B, Q, M, D)
    grad_close(torch.einsum("bqmd,bqmc->mdc", g4, samp).reshape(C, C), g64[3], g32[3], f"{tag} grad value_proj.weight")
    grad_close(torch.einsum("bqmd,bqm->md", g4, mass).reshape(C), g64[4], g32[4], f"{tag} grad value_proj.bias")
    for l in range(L):
        grad_close(grads[l], g64[5 + l], g32[5 + l], f"{tag} grad level {shapes[l]}")
    edge = torch.from_numpy((tt == -1) | (tt == SL.sizes_wh(shapes)[None, None, None, :, None, :]))
    assert edge.any() and (goff.cpu()[edge] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5, 6: the fused training block, atomics and scatter records
# ---------------------------------------------------------------------------------------------------------------------
_BLOCK_PARAMS = ["ms_deform_attn.sampling_offsets.weight", "ms_deform_attn.sampling_offsets.bias",
                 "ms_deform_attn.attention_weights.weight", "ms_deform_attn.attention_weights.bias",
                 "ms_deform_attn.value_proj.weight", "ms_deform_attn.value_proj.bias"]


@pytest.mark.parametrize("P", [1, 2, 4])
def test_training_block_on_the_lattice(P, monkeypatch):
    """train_fused.xattn_ffn_blocks, XF_SCATTER False (per-corner atomics, replicas of tiny maps) and True (scatter records +
    xf_scatter_small_kernel; with six small maps the largest keeps atomics), V = 2, L * P up to the limit of 20.
    sampling_offsets.weight = 0 and .bias = the offset lattice, so every query's offsets are exactly the bias; refs = the ref
    lattice.  y3, d refs WITH the kinks (the rule says which slope), every feature-map gradient, and the gradients of
    sampling_offsets / attention_weights / value_proj, all element by element against the fp64 oracle with the floor core."""
    from dpft_amd.models.fusers import train_fused as tf
    from dpft_amd.models.fusers.mpfusion import MLFusion
    from dpft_amd.models.layers.ms_deform_attn import make_pyramid_state as mk
    from oracle import dprt_oracle as O
    dev = torch.device("cuda", 0)
    shapes = SL.block_shapes(P)
    V, B, L = 2, 2, len(shapes)
    torch.manual_seed(300 + P)
    layers = [MLFusion(d_model=16, d_ffn=32, n_levels=L, n_heads=8, n_points=P, activation="Mish", dropout=0.0, norm=True)
              for _ in range(V)]
    refs_v, ts = [], []
    for v, ml in enumerate(layers):
        assert tf.xf_supported(ml)
        refs32, off32 = SL.block_lattice(shapes, P, v)
        Q = len(refs32)
        both = np.stack((refs32, refs32[::-1]))                                          # batch element 1 walks it backwards
        t32 = SL.replay_ref_off(both, np.broadcast_to(off32, (B, Q) + off32.shape), shapes).astype(np.float64)
        t = np.stack([SL.block_t(r, off32, shapes) for r in both])
        assert np.isfinite(off32).all() and np.abs(off32).max() <= SL.FAR
        assert np.array_equal(t32, t), "the block lattice is not exact in float32"       # cap on dropped points: 0
        SL.assert_coverage(t, shapes, far=64.0 if v == 0 else SL.FAR, what=f"block view {v}")
        a = ml.ms_deform_attn
        with torch.no_grad():
            a.sampling_offsets.weight.zero_()
            a.sampling_offsets.bias.copy_(torch.from_numpy(off32).reshape(-1))
            torch.nn.init.normal_(a.attention_weights.weight, 0.0, 0.3)
            torch.nn.init.normal_(a.attention_weights.bias, 0.0, 0.5)
            torch.nn.init.normal_(a.value_proj.bias, 0.0, 0.3)
        refs_v.append(torch.from_numpy(both))
        ts.append(t)
    layers = [ml.to(dev) for ml in layers]
    feats = [[(torch.randn(B, h, w, 16, device=dev) * 0.8).requires_grad_(True) for h, w in shapes] for _ in range(V)]
    y1 = (torch.randn(V, B, Q, 16, device=dev) * 0.7).requires_grad_(True)
    pos = (torch.randn(Q, 16, device=dev) * 0.5).requires_grad_(True)
    refs = torch.stack(refs_v).to(dev).requires_grad_(True)
    gy = torch.randn(V, B, Q, 16, device=dev)
    flat = [t_ for fv in feats for t_ in fv]
    by_name = [dict(ml.named_parameters()) for ml in layers]
    plist = [by_name[v][n] for v in range(V) for n in _BLOCK_PARAMS]
    seed = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch_seen = []
    real_call = tf.lib.call

    def spy(name, *args):
        if name == "dpft_xattn_ffn_train_bwd_f32":
            scratch_seen.append(args[-4])
        return real_call(name, *args)
    monkeypatch.setattr(tf.lib, "call", spy)
    res = {}
    for scatter in (False, True):
        monkeypatch.setattr(tf, "XF_SCATTER", scatter)
        out = tf.xattn_ffn_blocks(layers, [mk(fv) for fv in feats], y1, pos, refs, seed, 1, 0.0)
        res[scatter] = (out.detach().clone(), [g.detach().clone() for g in torch.autograd.grad(out, [refs] + flat + plist, gy)])
    assert len(scratch_seen) == 2 and scratch_seen[0] is None and scratch_seen[1], "XF_SCATTER=True did not take the record path"
    names = ["refs"] + [f"view {v} level {shapes[l]}" for v in range(V) for l in range(L)] + \
            [f"view {v} {n}" for v in range(V) for n in _BLOCK_PARAMS]

    def oracle(dt):
        c = lambda x: x.detach().to(dt).cpu().requires_grad_(True)
        y, p_, r = c(y1), c(pos), c(refs)
        fs = [[c(t_) for t_ in fv] for fv in feats]
        outs, leaves = [], []
        for v, ml in enumerate(layers):
            sd = {f"ml.{k}": c(t_) for k, t_ in ml.state_dict().items()}
            ca = O.ms_deform_attn(y[v] + p_.unsqueeze(0), r[v], fs[v], sd, "ml.ms_deform_attn", 8, P, core=O.msda_core_floor)
            y2 = O._ln(y[v] + ca, sd, "ml.norm2")
            ff = F.linear(F.mish(F.linear(y2, sd["ml.ffn1.weight"], sd["ml.ffn1.bias"])), sd["ml.ffn2.weight"], sd["ml.ffn2.bias"])
            outs.append(O._ln(y2 + ff, sd, "ml.norm3"))
            leaves += [sd["ml." + n] for n in _BLOCK_PARAMS]
        out = torch.stack(outs)
        return out.detach(), torch.autograd.grad(out, [r] + [t_ for fv in fs for t_ in fv] + leaves, gy.to(dt).cpu())
    (o64, g64), (o32, g32) = oracle(torch.float64), oracle(torch.float32)
    assert torch.equal(res[True][0], res[False][0])
    for scatter in (False, True):
        tag = f"block P{P} {'records' if scatter else 'atomics'}"
        fwd_close(res[scatter][0], o64, f"{tag} y3")
        for got, a, b, n in zip(res[scatter][1], g64, g32, names):
            where = (lambda idx: f" at ref {refs[idx[0], idx[1], idx[2]].tolist()}") if n == "refs" else None
            grad_close(got, a, b, f"{tag} d {n}", where)
    for a, b, n in zip(res[True][1], res[False][1], names):                              # the two paths, as in
        err = float((a - b).norm() / b.norm().clamp_min(1e-12))                         # test_xattn_ffn_backward_small_map_scatter_equals_atomics
        assert err < 2e-6, (n, err)


# ---------------------------------------------------------------------------------------------------------------------
# 7: the inference decoder
# ---------------------------------------------------------------------------------------------------------------------
def test_inference_decoder_reaches_every_zone_and_equals_the_eager_decoder(monkeypatch):
    """Small config model, sampling_offsets.weight = 0 and a bias that puts, on every level of every view, a sample into each
    of the nine zones, outside on all four sides and 2^20 pixels away; the fused inference decoder against the eager decoder
    (torch ops + ops.xattn_fwd), all four outputs element by element.  Forward only, so no exactness is needed: the sample
    positions are recomputed in fp64 from what the eager path's MSDeformAttn modules were given and the coverage is asserted
    on those."""
    from dpft_amd.configs import load_config
    from dpft_amd.models import build
    from dpft_amd.models.layers.ms_deform_attn import MSDeformAttn
    from dpft_amd.synthetic import make_batch
    cfg = copy.deepcopy(load_config("kradar"))
    cfg["model"]["backbones"]["camera_mono"]["name"] = "ResNet50"
    cfg["model"]["fuser"]["dropout"] = 0.0
    shapes_in = {"camera_mono": (96, 160, 3), "radar_bev": (128, 43, 6), "radar_front": (37, 107, 6)}
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(12)
    model = build("dprt", cfg)
    with torch.no_grad():
        for n, p in model.fuser.named_parameters():
            p.add_(torch.randn(p.shape, generator=g) * 0.05)
    model = model.to(DEV).eval()
    batch = make_batch(cfg["model"]["inputs"], 2, seed=11, shapes=shapes_in, device=DEV)
    fuser = model.fuser
    mods = {n: m for n, m in fuser.named_modules() if isinstance(m, MSDeformAttn)}
    seen = {}
    real = MSDeformAttn.forward_levels

    def hooked(self, query, reference_points, state, token):
        name = next(n for n, m in mods.items() if m is self)
        seen.setdefault(name, []).append((query.detach().double().cpu(), reference_points.detach().double().cpu(),
                                          [tuple(l.shape[1:3]) for l in state.levels]))
        return real(self, query, reference_points, state, token)
    monkeypatch.setattr(MSDeformAttn, "forward_levels", hooked)

    def eager():
        fuser.use_fused_inference = False
        monkeypatch.setattr(type(fuser), "use_fused_train", False)
        for layer in fuser.mpfusion.values():
            monkeypatch.setattr(type(layer), "use_fused_train", False)
        seen.clear()
        with torch.no_grad():
            return {k: v.clone() for k, v in model(batch).items()}
    eager()
    assert len(seen) == len(mods), "the eager decoder did not go through every MSDeformAttn module"
    # the first layer's reference points depend on the query grid and the projections only: aim the offsets at them
    targets = [(a, b) for a in (1, 2, 3) for b in (1, 2, 3)] + [(0, 2), (4, 2), (2, 0), (2, 4)]
    with torch.no_grad():
        for name, m in mods.items():
            view = name.split(".")[3]                      # mpfusion.fusion<i>.ml_fusion_layers.ms_deform_attn<v>.ms_deform_attn
            first = f"mpfusion.fusion0.ml_fusion_layers.{view}.ms_deform_attn"
            _, ref0, lv = seen[first][0]
            r0 = ref0[0, ref0.shape[1] // 2].numpy()                                      # one query of batch element 0
            off = np.zeros((m.n_heads, m.n_levels, m.n_points, 2))
            for l, (H, W) in enumerate(lv):
                size = np.array([W, H], np.float64)
                spread = np.linspace(-1.3, 1.3, m.n_heads * m.n_points)                   # from far outside to the far side
                slots = np.stack((spread * W, spread[::-1] * H), -1)
                zt = lambda z, s: {0: -1.5, 1: -0.5, 2: (s - 1) / 2, 3: s - 0.5, 4: s + 0.5}[z]
                for k, (zx, zy) in enumerate(targets):
                    slots[k] = np.array([zt(zx, W), zt(zy, H)]) + 0.5 - r0 * size
                slots[len(targets)] = (SL.FAR, -SL.FAR)
                slots[len(targets) + 1] = (-SL.FAR, 0.0)
                off[:, l] = slots.reshape(m.n_heads, m.n_points, 2)
            m.sampling_offsets.weight.zero_()
            m.sampling_offsets.bias.copy_(torch.from_numpy(off).reshape(-1).float())
    ref = eager()
    for name, calls in seen.items():
        m = mods[name]
        bias = m.sampling_offsets.bias.detach().double().cpu().view(m.n_heads, m.n_levels, m.n_points, 2)
        for query, rp, lv in calls:
            assert float(m.sampling_offsets.weight.abs().max()) == 0
            t = rp[:, :, None, None, None, :] * torch.tensor([[w, h] for h, w in lv], dtype=torch.float64)[None, None, None, :, None, :] \
                + bias[None, None] - 0.5
            assert torch.isfinite(t).all() and float(t.abs().max()) < 2 ** 21
            SL.assert_coverage(t.numpy(), lv, kinks=False, what=name)
    monkeypatch.undo()
    fuser.use_fused_inference = True
    with torch.no_grad():
        out = model(batch)
    assert fuser.__dict__.get("_fused_decoder"), "the fused inference decoder was not used"
    for k in ref:
        fwd_close(out[k], ref[k], f"inference decoder {k}")
