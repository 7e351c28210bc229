"""LearnableQueries on the GPU: the centre kernels (csrc/queries.hip), the backward of the iteration-0 reference points
(dpft_ref_points_bwd_f32), and the path of the parameter's gradient through the fused training decoder, the replayed decoder
graphs, the gradient buckets and the fused AdamW -- plus the inference side, where the centres must follow the parameter.

Every gradient gate is the project's 5e-4 relative L2 against fp64 (test_fused_head_block_vs_oracle,
test_product_fuser_grads_match_reference_golden: the same ref_point arithmetic)."""
import copy
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import dprt_oracle as O
from tests.test_gpu_model import SHAPES, _golden_fuser, close, rel_l2, small_config
from tests.test_oracle_golden import FUSER_CFG, _fuser_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = 5e-4
KRADAR_GRID = dict(resolution=[20, 20, 1], minimum=[4, -50, 0], maximum=[72, 50, 0], transformation="spher2cart")


def _spher2cart64(q, degrees):
    r, phi, roh = q.unbind(-1)
    if degrees:
        phi, roh = torch.deg2rad(phi), torch.deg2rad(roh)
    return torch.stack((r * torch.cos(phi) * torch.cos(roh), r * torch.sin(phi) * torch.cos(roh), r * torch.sin(roh)), -1)


# ---------------------------------------------------------------------------------------------------------------------
# 1. centre kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["identity", "radians", "degrees"])
def test_centre_kernels_vs_fp64(mode):
    """dpft_query_center_fwd_f32 / _bwd_f32 through LearnableQueries for every (B, Q) off and on the launch tiling.
    Forward: rtol 1e-6 elementwise, with an absolute floor of 1e-6 of the largest centre coordinate -- a component near zero
    (y at phi ~ 0) carries the ABSOLUTE error of the rounded angle, r * eps, not a relative one.  Backward: the 5e-4 gate, and
    the same bits on a second call (the batch is summed in a fixed order)."""
    from dpft_amd.models.queries.learnable import LearnableQueries
    from dpft_amd.models.utils.transformations import Spher2Cart
    gen = torch.Generator().manual_seed(3)
    for B in (1, 2, 3):
        for Q in (1, 3, 63, 64, 65, 257, 400):
            tr = None if mode == "identity" else Spher2Cart(dim=-1, degrees=mode == "degrees")
            mod = LearnableQueries([Q, 1, 1], [4, -50, -20], [72, 50, 20], transformation=tr)
            ang = 1.0 if mode == "degrees" else float(np.pi / 180)
            with torch.no_grad():
                mod.queries.copy_((torch.rand(Q, 3, generator=gen) * torch.tensor([68.0, 100 * ang, 40 * ang])
                                   + torch.tensor([4.0, -50 * ang, -20 * ang])))
            mod = mod.to(DEV)
            assert mod.kernel_mode() == {"identity": 0, "radians": 1, "degrees": 2}[mode]
            out = mod(torch.zeros(B, 1, device=DEV))["center"]
            assert tuple(out.shape) == (B, Q, 3) and out.grad_fn is not None and "QueryCenterFn" in type(out.grad_fn).__name__
            q64 = mod.queries.detach().double().cpu().requires_grad_(True)
            c64 = q64 if mode == "identity" else _spher2cart64(q64, mode == "degrees")
            ref = c64.unsqueeze(0).repeat(B, 1, 1)
            close(out, ref, rtol=1e-6, atol_scale=1e-6, what=f"centres {mode} B={B} Q={Q}")
            cot = torch.randn(B, Q, 3, generator=gen)
            (gref,) = torch.autograd.grad(ref, q64, cot.double())
            (g1,) = torch.autograd.grad(out, mod.queries, cot.to(DEV), retain_graph=True)
            (g2,) = torch.autograd.grad(out, mod.queries, cot.to(DEV))
            assert torch.equal(g1, g2), (mode, B, Q)
            e = rel_l2(g1, gref)
            assert e < GATE, (mode, B, Q, e)


# ---------------------------------------------------------------------------------------------------------------------
# 2. reference-point backward
# ---------------------------------------------------------------------------------------------------------------------
def _normalised_unclipped(center, T, P, shape, flag):
    """(u / W, v / H) before the clip, fp64 (mpfusion.py:617-696 without its last line)."""
    q = center
    if flag:
        hom = torch.cat((q, torch.ones_like(q[..., :1])), -1)
        p = torch.einsum("bij,bkj->bki", T, hom)
        q = torch.stack(O.cart2spher_deg(p[..., 0], p[..., 1], p[..., 2]), -1)
    hom = torch.cat((q, torch.ones_like(q[..., :1])), -1)
    p = torch.einsum("bij,bkj->bki", P, hom)
    w = p[..., 2]
    safe = torch.where(w != 0, w, torch.ones_like(w))
    return torch.stack((p[..., 0] / safe / shape[:, 1:2], p[..., 1] / safe / shape[:, 0:1]), -1)


def _projections(B, V, flags, gen, p_rows, stride):
    """The projection families of test_fused_head_block_vs_oracle (perturbed identity + translation under the flag, zero T
    otherwise; perspective and affine P), with 3- or 4-row P and (B, stride) int64 shape rows.  CPU fp32 tensors."""
    projection, shapes = [], []
    for v in range(V):
        T = torch.eye(4).repeat(B, 1, 1)
        if flags[v]:
            T[:, :3, :3] += torch.randn(B, 3, 3, generator=gen) * 0.05
            T[:, :3, 3] = torch.randn(B, 3, generator=gen)
        else:
            T.zero_()
        P = torch.zeros(B, 4, 4)
        P[:, 0, :] = torch.tensor([4.0, 1.5, 0.3, 60.0])
        P[:, 1, :] = torch.tensor([0.2, 0.4, 3.0, 40.0])
        P[:, 2, :] = torch.tensor([0.01, 0.0, 0.0, 1.0]) if v % 2 == 0 else torch.tensor([0.0, 0.0, 0.0, 1.0])
        P[:, 3, 3] = 1.0
        projection.append((T, P[:, :p_rows[v]].contiguous()))
        shapes.append(torch.tensor([[128 + 16 * v, 256 - 32 * v, 3][:stride]] * B, dtype=torch.int64))
    return projection, shapes


def _margin_centres(B, Q, projection, shapes, flags, gen, margin=1e-3):
    """Centres whose normalised points all lie at least `margin` inside (0,1) or at least `margin` outside it: rows that
    come closer to a clip edge in any view are drawn again.  Both sides then have a well-defined gradient (outside: exactly 0),
    and fp32 and fp64 agree on the side."""
    def draw(n):
        return torch.randn(n, 3, generator=gen) * torch.tensor([25.0, 14.0, 4.0]) + torch.tensor([30.0, 0.0, 0.0])
    c = draw(B * Q).view(B, Q, 3)
    for _ in range(50):
        bad = torch.zeros(B, Q, dtype=torch.bool)
        for (T, P), s, f in zip(projection, shapes, flags):
            n = _normalised_unclipped(c.double(), T.double(), P.double(), s.double(), f)
            bad |= ((n.abs() < margin) | ((n - 1).abs() < margin)).any(-1)
        if not bad.any():
            return c
        c[bad] = draw(int(bad.sum()))
    raise AssertionError("could not place the centres off the clip edges")


def _ref_points_grads(projection, shapes, flags, center, drefs):
    """RefPointsFn forward + backward on the device -> (refs, dcenter)."""
    from dpft_amd.models.fusers import train_fused as tf
    proj = tf._Proj([(t.to(DEV), p.to(DEV)) for t, p in projection], [s.to(DEV) for s in shapes], flags)
    c = center.to(DEV).requires_grad_(True)
    refs = tf.RefPointsFn.apply(proj, c)
    (dc,) = torch.autograd.grad(refs, c, drefs.to(DEV))
    return refs.detach(), dc


@pytest.mark.parametrize("B,Q,flags,p_rows,stride", [(2, 100, (0, 1, 1), (4, 3, 3), 3), (1, 33, (1, 0, 1, 0), (3, 4, 4, 3), 2),
                                                     (3, 65, (1,), (4,), 2), (2, 7, (0, 0, 1), (3, 3, 4), 3)])
def test_ref_points_bwd_vs_fp64(B, Q, flags, p_rows, stride):
    """dpft_ref_points_bwd_f32 == fp64 autograd of oracle.dprt_oracle.reference_points, summed over the views: V in {1, 3, 4},
    mixed has_t, 3- and 4-row P, shape rows of stride 2 and 3; every row takes part (see _margin_centres)."""
    V = len(flags)
    gen = torch.Generator().manual_seed(23 + Q)
    projection, shapes = _projections(B, V, flags, gen, p_rows, stride)
    center = _margin_centres(B, Q, projection, shapes, flags, gen)
    drefs = torch.randn(V, B, Q, 2, generator=gen)
    refs, dc = _ref_points_grads(projection, shapes, flags, center, drefs)
    c64 = center.double().requires_grad_(True)
    r64 = torch.stack([O.reference_points(c64, t.double(), p.double(), s[:, :2].double())
                       for (t, p), s in zip(projection, shapes)])
    (g64,) = torch.autograd.grad(r64, c64, drefs.double())
    inside = ((r64 > 0) & (r64 < 1)).float().mean()
    assert 0.05 < float(inside) < 0.999 or B * Q < 10, float(inside)      # both sides of the clip occur
    close(refs, r64, rtol=1e-4, atol_scale=1e-5, what="refs")
    e = rel_l2(dc, g64)
    print(f"ref_points_bwd B={B} Q={Q} V={V}: rel L2 {e:.3e}, inside the clip {float(inside):.2f}")
    assert e < GATE, e


def test_ref_points_bwd_pole_rows():
    """Rows at the poles of the rule: w == 0 and w < 0 (view 0, perspective P with an exactly representable zero), a centre
    that view 1's transformation maps to r == 0, two on its z axis (rho^2 == 0, |z / r| == 1, both signs).  Where fp64 autograd
    is defined (w == 0 takes the undivided coordinates, w < 0 divides) the rows meet the gate; at r == 0 / rho^2 == 0 torch
    gives NaN, the kernels' convention is a finite gradient: none through the norm / elevation / azimuth at r == 0 (the view
    adds exactly nothing), none through the azimuth on the z axis.  And on EVERY row the result is bit-equal to what
    hd_train_bwd_kernel hands back as dcenter_prev for the same centre (a head whose centre branch adds exactly zero)."""
    from dpft_amd.models.fusers import train_fused as tf
    from dpft_amd.models.fusers.mpfusion import MPFusion
    from dpft_amd.models.heads.detection import LinearDetectionHead
    B, Q, V, flags = 2, 37, 2, (0, 1)
    gen = torch.Generator().manual_seed(5)
    T1 = torch.eye(4).repeat(B, 1, 1)
    T1[:, :3, 3] = torch.tensor([1.0, -2.0, 0.5])
    P0 = torch.tensor([[4.0, 1.5, 0.3, 60.0], [0.2, 0.4, 3.0, 40.0], [0.5, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, 1.0]]).repeat(B, 1, 1)
    P1 = torch.tensor([[4.0, 1.5, 0.3, 60.0], [0.2, 0.4, 3.0, 40.0], [0.0, 0.0, 0.0, 1.0]]).repeat(B, 1, 1)
    projection = [(torch.zeros(B, 4, 4), P0), (T1, P1)]
    shapes = [torch.tensor([[128, 256]] * B), torch.tensor([[96, 512]] * B)]
    center = _margin_centres(B, Q, projection, shapes, flags, gen)
    poles = torch.tensor([[-2.0, 1.0, 0.25],        # 0: w == 0 in view 0
                          [-6.0, -60.0, -10.0],     # 1: w == -2 in view 0
                          [-1.0, 2.0, -0.5],        # 2: T1 c == 0: r == 0 in view 1
                          [-1.0, 2.0, 3.5],         # 3: T1 c == (0, 0, 4): z axis, z / r == 1
                          [-1.0, 2.0, -4.5]])       # 4: T1 c == (0, 0, -4): z / r == -1
    center[0, :5] = poles
    for (T, P), s, f in zip(projection, shapes, flags):      # rows 0, 1 keep the margin in both views (fp64 is compared there)
        n = _normalised_unclipped(center[:1, :2].double(), T[:1].double(), P[:1].double(), s[:1].double(), f)
        assert not ((n.abs() < 1e-3) | ((n - 1).abs() < 1e-3)).any(), n
    n0 = _normalised_unclipped(center[:1, :2].double(), projection[0][0][:1].double(), P0[:1].double(), shapes[0][:1].double(), 0)
    assert ((n0 > 0) & (n0 < 1)).all(), n0                  # ... and inside the clip in view 0: the w rule carries a gradient
    drefs = torch.randn(V, B, Q, 2, generator=gen)
    _, dc = _ref_points_grads(projection, shapes, flags, center, drefs)
    assert torch.isfinite(dc).all()
    # fp64 where it is defined: everything but rows 2-4 of batch 0
    c64 = center.double().requires_grad_(True)
    r64 = torch.stack([O.reference_points(c64, t.double(), p.double(), s.double()) for (t, p), s in zip(projection, shapes)])
    (g64,) = torch.autograd.grad(r64, c64, drefs.double())
    keep = torch.ones(B, Q, dtype=torch.bool)
    keep[0, 2:5] = False
    assert torch.isfinite(g64[keep]).all()
    assert rel_l2(dc.cpu()[keep], g64[keep]) < GATE
    assert rel_l2(dc.cpu()[0, :2], g64[0, :2]) < GATE and float(g64[0, :2].abs().min()) > 0
    # r == 0: view 1 adds exactly nothing -- the row equals the one-view result
    _, dc0 = _ref_points_grads(projection[:1], shapes[:1], flags[:1], center, drefs[:1])
    assert torch.equal(dc[0, 2], dc0[0, 2])
    # the head block's backward on the same centres
    torch.manual_seed(2)
    layer = MPFusion(V, d_model=16, d_ffn=32, n_levels=[2] * V, n_heads=[8] * V, n_points=[2] * V, activation="Mish",
                     norm=True, reduction="linear").to(DEV)
    head = LinearDetectionHead(16, 2, 3, 3).to(DEV)
    with torch.no_grad():
        head.layers["center_head"][6].weight.zero_()
    y3 = torch.randn(V, B, Q, 16, device=DEV)
    prev = center.to(DEV).requires_grad_(True)
    proj = tf._Proj([(t.to(DEV), p.to(DEV)) for t, p in projection], [s.to(DEV) for s in shapes], flags)
    _, out, refs = tf.head_block(layer, head, proj, y3, prev, True)
    assert torch.equal(out["center"].detach(), prev.detach())
    (dprev,) = torch.autograd.grad(refs, prev, drefs.to(DEV))
    assert torch.equal(dc, dprev), float((dc - dprev).abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# 3. fuser level
# ---------------------------------------------------------------------------------------------------------------------
def _oracle_impfusion(views, shapes, projections, center0, sd, detach_refs0=False):
    """oracle.dprt_oracle.impfusion, optionally with the iteration-0 reference points cut off the centres (what the fused
    branch computed before the querent could be learned)."""
    B = center0.shape[0]
    query = sd["fuser.query"].unsqueeze(0).repeat(B, 1, 1)
    qpos = sd["fuser.query_embedding.weight"].unsqueeze(0).repeat(B, 1, 1)
    out = OrderedDict(center=center0)
    for it in range(FUSER_CFG["i_iter"]):
        c = out["center"].detach() if (it == 0 and detach_refs0) else out["center"]
        refs = [O.reference_points(c[..., :3], t, p, s) for (t, p), s in zip(projections, shapes)]
        query = O.mpfusion(query, views, refs, qpos, sd, f"fuser.mpfusion.fusion{it}", FUSER_CFG["n_heads"],
                           FUSER_CFG["n_points"], FUSER_CFG["activation"])
        out = O.detection_head(query, out["center"], sd, f"fuser.heads.{it}")
    return out


@pytest.fixture(scope="module")
def oracle64(golden):
    """fp64 oracle on fuser_small.npz with the fixture's queries: outputs, queries.grad for the cotangent sets A and B, the same
    with the iteration-0 reference points detached, and for A the gradient of every decoder parameter and pyramid level.
    Computed once."""
    g, gg, gq = golden("fuser_small.npz"), golden("fuser_grads.npz"), golden("learnable_queries.npz")
    sd, views, proj, shp = _fuser_inputs(g)
    d = lambda t: t.double() if t.is_floating_point() else t      # noqa: E731
    sd = {k: d(v).requires_grad_(True) for k, v in sd.items()}
    views = [[d(l).requires_grad_(True) for l in lv] for lv in views]
    proj = [(d(t), d(p)) for t, p in proj]
    cot = {k: torch.from_numpy(gg[f"cot/{k}"]).double() for k in ("center", "size", "angle", "class")}
    res = {}
    for detach in (False, True):
        q = torch.from_numpy(gq["queries"]).double().requires_grad_(True)
        out = _oracle_impfusion(views, shp, proj, _spher2cart64(q, True).unsqueeze(0).repeat(2, 1, 1), sd, detach)
        for tag in ("A", "B"):
            loss = sum((out[k] * cot[k]).sum() for k in out if not (tag == "B" and k == "center"))
            (res[(tag, detach)],) = torch.autograd.grad(loss, q, retain_graph=True)
        if not detach:
            res["out"] = {k: v.detach() for k, v in out.items()}
            loss = sum((out[k] * cot[k]).sum() for k in out)
            names = list(sd) + [f"view/{vi}/{l}" for vi in range(3) for l in range(5)]
            grads = torch.autograd.grad(loss, list(sd.values()) + [l for lv in views for l in lv], allow_unused=True)
            res["others_A"] = {n: t for n, t in zip(names, grads) if t is not None}
    return res


def _graph_has(t, name):
    seen, todo = set(), [t.grad_fn]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        if name in type(f).__name__:
            return True
        todo += [n for n, _ in f.next_functions]
    return False


def _fixture_querent(golden):
    from dpft_amd.models.queries import build_querent
    q = build_querent("learnable_querent", dict(KRADAR_GRID))
    q.load_state_dict({"queries": torch.from_numpy(golden("learnable_queries.npz")["queries"])})
    return q.to(DEV)


def test_oracle_notices_the_missing_reference_point_term(oracle64):
    """Cotangent set B (no cotangent on the centres) is the discriminating one: without the term through the iteration-0
    reference points the gradient is off by far more than the gate can hide."""
    full, cut = oracle64[("B", False)], oracle64[("B", True)]
    assert rel_l2(cut, full) > 100 * GATE, rel_l2(cut, full)
    print("detached refs0: rel L2 B", rel_l2(cut, full), "A", rel_l2(oracle64[("A", True)], oracle64[("A", False)]))


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("tag", ["A", "B"])
def test_fuser_queries_grad_matches_reference_and_fp64(golden, oracle64, tag, fused):
    """queries.grad through the product IMPFusion (fused training kernels; and with IMPFusion.use_fused_train off, where
    autograd differentiates get_reference_points) against the reference's own (fixture) and the fp64 oracle.  With the fused
    kernels and set A every other parameter and pyramid gradient is held to the fp64 oracle at the same gate (fuser_grads.npz
    cannot serve here: it was recorded on the static querent's centres, and the loss is a different one on the learned ones)."""
    from dpft_amd.models.fusers import train_fused as tf
    g, T, fuser, views, proj, shp = _golden_fuser(golden, 0.0)
    gg, gq = golden("fuser_grads.npz"), golden("learnable_queries.npz")
    fuser.train()
    fuser.use_fused_train = fused
    querent = _fixture_querent(golden)
    views = [OrderedDict((k, v.clone().requires_grad_(True)) for k, v in lv.items()) for lv in views]
    out = fuser(batch=views, shape=shp, projection=proj, out=querent(torch.zeros(2, 1, device=DEV)))
    layers = list(fuser.mpfusion.values())
    assert all(l.fused_blocks_supported() and tf.head_supported(l, h) for l, h in zip(layers, fuser.heads))
    assert _graph_has(out["center"], "RefPointsFn") == fused and _graph_has(out["center"], "QueryCenterFn")
    cot = {k: T(gg[f"cot/{k}"]).to(DEV) for k in out}
    if tag == "B":
        cot["center"] = torch.zeros_like(cot["center"])
    loss = sum((out[k] * cot[k]).sum() for k in out)
    if tag == "A":      # (B's loss is a small difference of large sums: the gradients are what is compared there)
        close(loss, T(gq["loss_A"]), rtol=1e-4, what="loss")
    loss.backward()
    e_ref, e_64 = rel_l2(querent.queries.grad, T(gq[f"grad_{tag}"])), rel_l2(querent.queries.grad, oracle64[(tag, False)])
    print(f"queries.grad {tag} fused={fused}: vs reference {e_ref:.3e}, vs fp64 {e_64:.3e}")
    assert e_ref < GATE and e_64 < GATE, (e_ref, e_64)
    if tag == "A" and fused:
        others = oracle64["others_A"]
        params = {"fuser." + k: p for k, p in fuser.named_parameters()}
        assert len([k for k in others if k in params]) > 200 and all(("grad/" + k[6:]) in gg for k in others if k in params)
        for k, p in params.items():
            if k in others:
                e = rel_l2(p.grad, others[k])
                assert e < GATE or float(others[k].norm()) < 1e-9, (k, e)
        for vi in range(3):
            for l in range(5):
                e = rel_l2(views[vi][str(l)].grad, others[f"view/{vi}/{l}"])
                assert e < GATE, (vi, l, e)


# ---------------------------------------------------------------------------------------------------------------------
# 5a. inference, fuser level
# ---------------------------------------------------------------------------------------------------------------------
def test_fused_inference_decoder_with_learned_centres_matches_oracle(golden, oracle64):
    g, T, fuser, views, proj, shp = _golden_fuser(golden, 0.1)
    querent = _fixture_querent(golden)
    fuser.eval()
    with torch.no_grad():
        out = fuser(batch=views, shape=shp, projection=proj, out=querent(torch.zeros(2, 1, device=DEV)))
    assert fuser.__dict__.get("_fused_decoder"), "the fused inference decoder did not run"
    for k in ("center", "size", "angle", "class"):
        close(out[k], oracle64["out"][k], rtol=1e-4, what=f"inference decoder {k}")
    assert torch.equal(out["class"].argmax(-1).cpu(), oracle64["out"]["class"].argmax(-1))


# ---------------------------------------------------------------------------------------------------------------------
# 4. - 6. the small model: replayed decoder graphs, gradient buckets, fused AdamW, inference after weight changes
# ---------------------------------------------------------------------------------------------------------------------
def _learned_config():
    cfg = small_config(dropout=0.0)
    cfg["model"]["querent"] = dict(KRADAR_GRID, name="learnable_querent", q_init="uniform_")
    return cfg


def _batch():
    from dpft_amd.synthetic import make_batch, make_labels
    cfg = _learned_config()
    return make_batch(cfg["model"]["inputs"], 2, seed=9, shapes=SHAPES, device=DEV), make_labels(2, seed=9, device=DEV)


@pytest.fixture(scope="module")
def base_model():
    from dpft_amd.models import build
    from tests.test_gpu_model import randomise_decoder
    torch.manual_seed(0)
    model = build("dprt", _learned_config())
    randomise_decoder(model, torch.Generator().manual_seed(4))
    return model


def _cotangent_step(model, batch, cot):
    """One forward + backward under fixed cotangents -> (outputs, queries.grad)."""
    model.zero_grad(set_to_none=True)
    out = model(batch)
    sum((out[k] * cot[k]).sum() for k in out).backward()
    return {k: v.detach().clone() for k, v in out.items()}, model.querent.queries.grad.detach().clone()


def test_graphed_decoder_follows_the_parameter(base_model):
    """GraphedFuser with a learned querent: two steps with an in-place change of querent.queries between them (an optimizer
    step) against the un-graphed fused path on the same weights.  A graph that kept the first step's centres as a constant
    would repeat step 1's outputs in step 2 and hand no gradient to the parameter."""
    batch, _ = _batch()
    plain = copy.deepcopy(base_model).to(DEV).train()
    graphed = copy.deepcopy(base_model).to(DEV).train()
    graphed.enable_fuser_graph(batch)
    g = graphed.__dict__["_graphed_fuser"]
    assert g.first_diff == 0 and g.static_inputs[0].requires_grad and g.static_grad_inputs[0] is not None
    gen = torch.Generator().manual_seed(8)
    cot = {k: torch.randn(s, generator=gen).to(DEV) for k, s in
           (("center", (2, 400, 3)), ("size", (2, 400, 3)), ("angle", (2, 400, 2)), ("class", (2, 400, 2)))}
    step = torch.tensor([3.0, 5.0, 0.0], device=DEV)
    outs = []
    for it in range(2):
        o_p, g_p = _cotangent_step(plain, batch, cot)
        o_g, g_g = _cotangent_step(graphed, batch, cot)
        assert graphed.__dict__["_graphed_fuser"] is g and g.last_inputs is not None
        for k in o_p:
            e = rel_l2(o_g[k], o_p[k])
            assert e < GATE, (it, k, e)
        e = rel_l2(g_g, g_p)
        print(f"graphed step {it}: queries.grad rel L2 {e:.3e} (|g| {float(g_p.norm()):.3e})")
        assert e < GATE and float(g_p.norm()) > 0, (it, e)
        outs.append(o_g)
        with torch.no_grad():
            for m in (plain, graphed):
                m.querent.queries.add_(step)
    assert rel_l2(outs[1]["center"], outs[0]["center"]) > 1e-2, "step 2 ran on step 1's centres"
    # the eval replay takes this call's centres as well
    with torch.no_grad():
        c_now = graphed.querent(batch)["center"]
        feats = graphed._encode_views(batch)
        shapes = {i: batch[f"{i}_shape"] for i in graphed.inputs}
        o_e = g(feats, shapes, graphed._get_projetions(graphed.inputs, batch), OrderedDict(center=c_now))
        assert torch.equal(g.eval_inputs[0], c_now)
        graphed.querent.queries.add_(step)
        c_next = graphed.querent(batch)["center"]
        o_e2 = g(feats, shapes, graphed._get_projetions(graphed.inputs, batch), OrderedDict(center=c_next))
        assert rel_l2(o_e2["center"], o_e["center"]) > 1e-2


@pytest.fixture(scope="module")
def trainer(base_model):
    """DataParallelTrainer on the small model with a learned querent: decoder graphs adding into the gradient buckets
    (grad_direct), FusedAdamW with clipping and an EMA."""
    from dpft_amd.training.trainer import DataParallelTrainer
    cfg = _learned_config()
    cfg["train"]["optimizer"]["lr"] = 1e-2
    cfg["train"]["clip_grad_norm"] = 0.1
    cfg["train"]["ema"] = {"decay": 0.9, "warmup": True}
    batch, labels = _batch()
    tr = DataParallelTrainer(copy.deepcopy(base_model), cfg, torch.device(DEV))
    tr.enable_graphs(batch)
    return tr, cfg, batch, labels


def test_train_step_moves_the_queries_through_buckets_clip_and_ema(base_model, trainer):
    """The parameter's gradient arrives in its bucket from the replayed decoder (grad_direct) as the un-graphed trainer computes
    it; one full step with FusedAdamW, clipping on: the parameter takes part in the norm, moves, and has its EMA; the step's loss
    equals that of the same weights with the querent on its torch ops (repeat + Spher2Cart) at 1e-5."""
    from dpft_amd.training.optimizer import FusedAdamW
    from dpft_amd.training.trainer import DataParallelTrainer
    tr, cfg, batch, labels = trainer
    assert isinstance(tr.optimizer, FusedAdamW)
    p = tr.model.querent.queries
    q0 = p.detach().clone()

    def grads_of(t):
        t.model.train()
        t.reducer.reset()
        loss, _ = t.loss_fn(t.model(batch), labels)
        loss.backward()
        t.reducer.finish()
        return float(loss.detach()), t.model.querent.queries.grad

    plain = DataParallelTrainer(copy.deepcopy(base_model), cfg, torch.device(DEV))
    l_plain, g_plain = grads_of(plain)
    l_graph, g_graph = grads_of(tr)
    assert tr.model.__dict__["_graphed_fuser"].grad_direct is tr.reducer
    assert g_graph.data_ptr() == tr.reducer.grad_buffer(p).data_ptr() and id(p) in tr.reducer.seen_ids()
    e = rel_l2(g_graph, g_plain)
    print(f"bucket gradient of querent.queries: rel L2 {e:.3e}, |g| {float(g_plain.norm()):.3e}")
    assert e < GATE and float(g_plain.norm()) > 0
    # the torch-op querent on the same weights
    eager = copy.deepcopy(base_model).to(DEV).train()
    eager.querent.kernel_mode = lambda: None
    out_e = eager(batch)
    assert "QueryCenterFn" not in str(type(eager.querent(batch)["center"].grad_fn))
    l_eager = float(plain.loss_fn(out_e, labels)[0])
    loss, _ = tr.train_step(batch, labels)
    torch.cuda.synchronize()
    assert abs(float(loss) - l_eager) <= 1e-5 * abs(l_eager), (float(loss), l_eager, l_plain, l_graph)
    assert not torch.equal(p.detach(), q0), "the fused AdamW did not move querent.queries"
    assert id(p) in tr.reducer.seen_ids()
    total = torch.sqrt(sum((q.grad.double() ** 2).sum() for q in tr.model.parameters() if q.grad is not None))
    assert abs(float(tr.last_grad_norm) - float(total)) <= 1e-4 * float(total), (float(tr.last_grad_norm), float(total))
    assert float(p.grad.norm()) > 0
    live = [q for q in tr.model.parameters() if q.requires_grad]
    ema = tr.ema_parameters()[[id(q) for q in live].index(id(p))]
    assert ema.shape == p.shape and torch.isfinite(ema).all()
    assert not torch.equal(ema, q0) and not torch.equal(ema, p.detach())
    lo, hi = torch.minimum(q0, p.detach()), torch.maximum(q0, p.detach())
    assert bool(((ema >= lo - 1e-5) & (ema <= hi + 1e-5)).all()), "the EMA lies between the old and the new parameter"


def _eval(model, batch):
    model.eval()
    with torch.no_grad():
        return {k: v.clone() for k, v in model(batch).items()}


def _fresh_like(model):
    """A newly built model with the same weights and buffers: no cache has seen any earlier value."""
    from dpft_amd.models import build
    fresh = build("dprt", _learned_config()).to(DEV)
    fresh.load_state_dict(model.state_dict())
    return fresh


def test_eval_forward_follows_optimizer_step_load_state_dict_and_ema_swap(trainer):
    """The no_grad centres are kept between calls; after the fused AdamW (raw-pointer writes), load_state_dict and swap_ema
    the eval forward must run on the new ones: compared with a freshly built model on the same weights."""
    from dpft_amd.hip.lib import note_weights_changed
    tr, cfg, batch, labels = trainer
    model = tr.model
    before = _eval(model, batch)                               # fills every weight-derived cache
    assert model.fuser.__dict__.get("_fused_decoder"), "the fused inference decoder did not run"
    kept = model.querent.__dict__["_centers"][1]
    with torch.no_grad():
        assert model.querent(batch)["center"] is kept
    tr.train_step(batch, labels)
    got = _eval(model, batch)
    want = _eval(_fresh_like(model), batch)
    for k in want:
        close(got[k], want[k], rtol=1e-4, atol_scale=1e-4, what=f"after optimizer.step {k}")
    assert rel_l2(got["center"], before["center"]) > 1e-4, "the step did not change the outputs"
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd["querent.queries"] = sd["querent.queries"] + torch.tensor([2.0, -4.0, 0.0], device=DEV)
    model.load_state_dict(sd)
    got2 = _eval(model, batch)
    want2 = _eval(_fresh_like(model), batch)
    for k in want2:
        close(got2[k], want2[k], rtol=1e-4, atol_scale=1e-4, what=f"after load_state_dict {k}")
    assert rel_l2(got2["center"], got["center"]) > 1e-3
    twin = copy.deepcopy(model)
    for q, e in zip([q for q in twin.parameters() if q.requires_grad], tr.ema_parameters()):
        q.data.copy_(e)
    note_weights_changed()
    want3 = _eval(_fresh_like(twin), batch)
    model.eval()
    with tr.ema_weights(), torch.no_grad():
        got3 = {k: v.clone() for k, v in model(batch).items()}
    for k in want3:
        close(got3[k], want3[k], rtol=1e-4, atol_scale=1e-4, what=f"under swap_ema {k}")
    assert rel_l2(got3["center"], got2["center"]) > 1e-5, "the EMA forward must differ from the live one"
    back = _eval(model, batch)
    for k in got2:
        close(back[k], got2[k], rtol=1e-4, atol_scale=1e-4, what=f"after swapping back {k}")


def test_rccl_one_rank_forced_collectives_with_learned_querent():
    """The forced-collectives one-rank path of tests/test_gpu_distributed.py (tools/rccl1_forced.py, decoder graphs on) with
    the learned querent: its gradient reaches its bucket before the bucket's all-reduce and the fused AdamW moves it."""
    env = dict(os.environ, GRAPHS="1", WIRE="fp32", QUERENT="learnable", HSA_ENABLE_IPC_MODE_LEGACY="0")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rccl1_forced.py")], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "rccl1 forced-collectives OK" in res.stdout and "learned querent OK" in res.stdout
