"""The bilinear sampling rule, once, in fp64 (oracle.dprt_oracle.msda_core_floor), pinned on the CPU:

  t = loc * size - 0.5;  a sample counts iff -1 < t < size on both axes, strictly;  floor;  four corners, each with its own
  in-map mask (zero padding);  backward = the slope of the cell [floor(t), floor(t) + 1): right-hand at an integer t, 0 for
  t <= -1 and t >= size.

Every HIP sampler restates this rule (tests/test_gpu_sampler_edges.py holds them to it element by element).  The grid_sample
formulation ``msda_core`` the golden fixtures were made with agrees with it in the forward and in every gradient EXCEPT the
location gradient on t == -1 exactly (grid_sample: one-sided slope from inside; the rule: 0); that set is pinned here."""
import numpy as np
import torch

from oracle import dprt_oracle as O
from tests import sampler_lattice as SL

CPU_SHAPES = [(1, 1), (1, 8), (4, 1), (2, 2), (8, 16)]


def _lattice_case(shapes, M=1, D=1, P=1, seed=3):
    g = torch.Generator().manual_seed(seed)
    t = SL.lattice_t(shapes, M, P)
    loc = torch.from_numpy((t + 0.5) / SL.sizes_wh(shapes)[None, None, :, None, :])[None]        # (1, Q, M, L, P, 2) fp64
    Q, L = t.shape[0], len(shapes)
    S = sum(h * w for h, w in shapes)
    value = torch.randn(1, S, M, D, generator=g, dtype=torch.float64)
    attn = torch.rand(1, Q, M, L, P, generator=g, dtype=torch.float64) + 0.25
    go = torch.randn(1, Q, M * D, generator=g, dtype=torch.float64)
    return t, value, loc, attn, go


def _lsi(shapes):
    return [0] + list(np.cumsum([h * w for h, w in shapes])[:-1])


def test_lattice_is_exact_in_fp32_and_covers_every_zone():
    """The kernels' own formula (loc * size - 0.5 in float32) reproduces the intended t bit for bit on power-of-two maps,
    +-2^20 pixels included, for the direct form and for the ref + off / size form; no point is dropped."""
    for M, P in ((1, 1), (3, 4)):
        t = SL.lattice_t(SL.POW2_SHAPES, M, P)
        assert np.isfinite(t).all() and np.abs(t).max() == SL.FAR
        assert np.array_equal(SL.replay_direct(SL.direct_loc(t, SL.POW2_SHAPES), SL.POW2_SHAPES).astype(np.float64), t)
        ref, off = SL.ref_off_split(t, SL.POW2_SHAPES)
        assert np.array_equal(SL.replay_ref_off(ref, off, SL.POW2_SHAPES).astype(np.float64), t)
        SL.assert_coverage(t, SL.POW2_SHAPES, what=f"M={M} P={P}")
    for P in (1, 2, 4):
        shapes = SL.block_shapes(P)
        ts = []
        for view in (0, 1):
            refs, off = SL.block_lattice(shapes, P, view)
            t32 = SL.replay_ref_off(refs, np.broadcast_to(off, (len(refs),) + off.shape), shapes)
            ts.append(SL.block_t(refs, off, shapes))
            assert np.array_equal(t32.astype(np.float64), ts[-1]), (P, view)
            SL.assert_coverage(ts[-1], shapes, far=64.0 if view == 0 else SL.FAR, what=f"block P={P} view {view}")
    # the odd pyramid: no kinks, so float32 rounding of loc cannot move a sample into another cell or zone
    t = SL.lattice_t(SL.ODD_SHAPES, 3, 4, kinks=False)
    t32 = SL.replay_direct(SL.direct_loc(t, SL.ODD_SHAPES), SL.ODD_SHAPES).astype(np.float64)
    assert np.array_equal(np.floor(t32), np.floor(t))
    for l, (H, W) in enumerate(SL.ODD_SHAPES):
        assert np.array_equal(SL.zone(t32[:, :, l, :, 0], W), SL.zone(t[:, :, l, :, 0], W))
        assert np.array_equal(SL.zone(t32[:, :, l, :, 1], H), SL.zone(t[:, :, l, :, 1], H))
    SL.assert_coverage(t, SL.ODD_SHAPES, kinks=False, what="odd pyramid")


def test_floor_core_equals_scalar_restatement():
    """msda_core_floor == the pure-python restatement of the upstream thread body, on the lattice and on random locations."""
    t, value, loc, attn, _ = _lattice_case(CPU_SHAPES)
    a = O.msda_core_floor(value, CPU_SHAPES, loc, attn)
    b = O.msda_core_scalar(value, CPU_SHAPES, _lsi(CPU_SHAPES), loc, attn)
    torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)
    gen = torch.Generator().manual_seed(0)                                   # the case of test_msda_core_vs_scalar_restatement
    shapes, lsi = [(5, 7), (3, 4), (1, 2)], [0, 35, 47]
    N, M, D, Lq, L, P = 2, 2, 2, 3, 3, 2
    value = torch.randn(N, 49, M, D, generator=gen, dtype=torch.float64)
    loc = torch.rand(N, Lq, M, L, P, 2, generator=gen, dtype=torch.float64) * 1.4 - 0.2
    attn = torch.rand(N, Lq, M, L, P, generator=gen, dtype=torch.float64)
    torch.testing.assert_close(O.msda_core_floor(value, shapes, loc, attn), O.msda_core_scalar(value, shapes, lsi, loc, attn),
                               rtol=1e-12, atol=1e-12)


def _grads(core, shapes, value, loc, attn, go):
    v, l, a = (x.clone().requires_grad_(True) for x in (value, loc, attn))
    out = core(v, shapes, l, a)
    gv, gl, ga = torch.autograd.grad(out, (v, l, a), go)
    return out.detach(), gv, gl, ga


def test_floor_core_vs_grid_sample_core_differs_only_on_t_equal_minus_one():
    """Forward, value gradient and attention gradient of the two cores agree to 1e-12 on the whole lattice; the location
    gradient agrees everywhere except on entries whose own axis sits on t == -1 exactly -- the one documented difference
    (sampling rule), and there on every entry whose other axis is inside the map (where grid_sample's one-sided
    slope is not 0 anyway): 21 165 (point, level) pairs, 633 differing entries with this lattice's repetition of the small
    levels."""
    t, value, loc, attn, go = _lattice_case(CPU_SHAPES)
    f = _grads(O.msda_core_floor, CPU_SHAPES, value, loc, attn, go)
    g = _grads(O.msda_core, CPU_SHAPES, value, loc, attn, go)
    for a, b, n in zip(f, g, ("out", "grad value", "grad loc", "grad attn")):
        if n != "grad loc":
            torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12, msg=lambda m: f"{n}: {m}")
    differ = ((f[2] - g[2]).abs() > 1e-9)[0].numpy()                         # (Q, M, L, P, 2)
    on_edge = t == -1
    assert t.shape[0] * t.shape[2] == 21165
    assert differ.any(), "grid_sample and the floor rule are expected to differ on t == -1"
    assert not (differ & ~on_edge).any(), "the two cores differ away from t == -1"
    wh = SL.sizes_wh(CPU_SHAPES)[None, None, :, None, :]
    inside = (t > -1) & (t < wh)
    expected = on_edge & inside[..., ::-1]                                   # own axis on -1, the other axis inside
    assert np.array_equal(differ, expected)
    assert int(differ.sum()) == 633, int(differ.sum())
    assert (f[2][0].numpy()[on_edge] == 0).all(), "the rule's location gradient on t == -1 is 0"


def test_floor_core_location_gradient_is_the_right_hand_difference_quotient():
    """d out / d t from autograd == (f(t + h) - f(t)) / h with h = 2^-10 px per axis at every lattice point with t != -1 (the
    function is linear along an axis inside a cell, so the quotient is exact up to rounding), and == 0 on t == -1."""
    t, value, loc, attn, go = _lattice_case(CPU_SHAPES)
    _, _, gl, _ = _grads(O.msda_core_floor, CPU_SHAPES, value, loc, attn, go)
    wh = torch.from_numpy(SL.sizes_wh(CPU_SHAPES))[None, None, None, :, None, :]
    gt = (gl / wh)[0].numpy()                                                # gradient with respect to t (pixels)
    h = 2.0 ** -10
    with torch.no_grad():
        f0 = O.msda_core_floor(value, CPU_SHAPES, loc, attn)
    L = len(CPU_SHAPES)
    # one (level, axis) at a time: out sums over levels, so stepping one level's axis isolates that entry (M = P = 1)
    for l in range(L):
        for ax in range(2):
            step = torch.zeros_like(loc)
            step[:, :, :, l, :, ax] = h / float(wh[0, 0, 0, l, 0, ax])
            with torch.no_grad():
                f1 = O.msda_core_floor(value, CPU_SHAPES, loc + step, attn)
            quot = ((f1 - f0) * go).sum(-1)[0].numpy() / h                   # (Q,)
            got = gt[:, 0, l, 0, ax]
            edge = t[:, 0, l, 0, ax] == -1
            far = np.abs(t[:, 0, l, 0]).max(-1) >= SL.FAR                    # far outside: no slope
            scale = max(float(np.abs(quot[~edge]).max()), 1e-30)
            assert np.abs(got - quot)[~edge].max() <= 1e-9 * scale, (l, ax, float(np.abs(got - quot)[~edge].max()), scale)
            assert (got[edge] == 0).all() and edge.any()
            assert (got[far] == 0).all()
