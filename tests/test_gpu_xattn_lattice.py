"""The training decoder's deformable cross-attention + FFN block (dpft_amd/csrc/decoder_train_x.hip: xf_train_fwd_kernel,
xf_train_bwd_kernel<true> and <false>, xf_scatter_small_kernel) against the fp64 oracle over the lattice of tests/xattn_lattice.py,
element by element: y3, d y1, d pos, d refs, every map gradient and all 16 parameter gradients of every view; through
train_fused.xattn_ffn_blocks with per-corner atomics (replicas of tiny maps) and with scatter records, through the two C entries
with saved == NULL, and through the backward entry with a replicated and a recorded map in one call.  The CPU half
(tests/test_xattn_lattice.py) shows that the table reaches what it names and that its inputs hold no kink.

Gates: the forward under tests.decoder_lattice.tolerance, every gradient under grad_close of tests/test_gpu_sampler_edges.py (4 x
the fp32 CPU oracle's own distance from fp64 for that tensor, floored at the forward rule).  Nothing is measured against a
kernel's own output.  Every figure is printed before it is asserted (``XATTN-LATTICE`` lines: |hip - fp64| over the gate, the
worst tensor of each class)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import xattn_lattice as L
from tests.test_gpu_sampler_edges import grad_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
_LAYERS = {}


def _layers(c):
    """The case's MLFusion layers on the device, built once (the weights are never changed)."""
    if c.name not in _LAYERS:
        from dpft_amd.models.fusers import train_fused as tf
        from dpft_amd.models.fusers.mpfusion import MLFusion
        out = []
        for (nl, P), p in zip(c.lp, L.cached(c)["params"]):
            ml = MLFusion(d_model=16, d_ffn=32, n_levels=nl, n_heads=8, n_points=P, activation="Mish", dropout=c.p_drop, norm=True)
            named = dict(ml.named_parameters())
            with torch.no_grad():
                for k, t in p.items():
                    assert named[k].shape == t.shape, (c.name, k)
                    named[k].copy_(t)
            ml = ml.to(DEV)
            assert tf.xf_supported(ml)
            named = dict(ml.named_parameters())
            assert all(a is b for a, b in zip(tf.view_params(ml)[6:], [named[k] for k in L.PARAMS]))
            out.append(ml)
        _LAYERS[c.name] = out
    return _LAYERS[c.name]


def _fwd_close(got, ref, what):
    """tests.decoder_lattice.tolerance, element-wise; the message names the worst element."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all(), what
    ratio = (got - ref).abs() / L.tolerance(ref)
    i = tuple(int(v) for v in np.unravel_index(int(ratio.argmax()), ref.shape))
    print(f"{what:44s} max|hip - fp64| {float((got - ref).abs().max()):.3e}   over the gate {float(ratio.max()):.4f}")
    assert float(ratio.max()) <= 1.0, f"{what}: worst element {i}: got {float(got[i])!r} ref {float(ref[i])!r}"
    return float(ratio.max())


def _gate(c, si, tag, y3, grads):
    """y3 and {name: gradient} under the two gates; prints every figure, then the worst ratio of each tensor class."""
    r64, r32 = L.cached_reference(c, torch.float64, si), L.cached_reference(c, torch.float32, si)
    worst, failed = {}, []
    if y3 is not None:
        worst["y3"] = _fwd_close(y3, r64["y3"], f"{tag} y3")
    for n, got in grads.items():
        a, b = r64["grads"][n], r32["grads"][n]
        k = L.tensor_class(n)
        worst[k] = max(worst.get(k, 0.0), L.gate_ratio(got, a, b))
        try:
            grad_close(got, a, b, f"{tag} d {n}")
        except AssertionError as e:                                  # every tensor is printed before the first failure is raised
            failed.append(str(e))
    print(f"XATTN-LATTICE {L.run_id((c, si)):18s} {tag:12s} " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert not failed, "\n".join(failed)


def _seed(c, si):
    return torch.full((1,), c.seeds[si], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("run", L.RUNS, ids=L.run_id)
def test_block_on_the_lattice(run, monkeypatch):
    """train_fused.xattn_ffn_blocks with XF_SCATTER False (atomics; maps of up to 256 pixels in 32 replicas) and True (scatter
    records + xf_scatter_small_kernel): the same forward bit for bit, and everything under the gates in both."""
    from dpft_amd.models.fusers import train_fused as tf
    from dpft_amd.models.layers.ms_deform_attn import make_pyramid_state as mk
    c, si = run
    inp, layers = L.cached(c), _layers(c)
    plist = [t for ml in layers for t in tf.view_params(ml)[6:]]
    seen = []
    real_call = tf.lib.call

    def spy(name, *args):
        if name == "dpft_xattn_ffn_train_bwd_f32":
            seen.append((args[-4], args[11]))                        # scratch, saved
        return real_call(name, *args)
    monkeypatch.setattr(tf.lib, "call", spy)
    res = {}
    for scatter in (False, True):
        monkeypatch.setattr(tf, "XF_SCATTER", scatter)
        leaf = lambda t: t.to(DEV).requires_grad_(True)              # noqa: E731
        y1, pos, refs = leaf(inp["y1"]), leaf(inp["pos"]), leaf(inp["refs"])
        feats = [[leaf(t) for t in fv] for fv in inp["feats"]]
        out = tf.xattn_ffn_blocks(layers, [mk(fv) for fv in feats], y1, pos, refs, _seed(c, si), c.salt, c.p_drop)
        grads = torch.autograd.grad(out, [y1, pos, refs] + [t for fv in feats for t in fv] + plist, inp["gy"].to(DEV))
        torch.cuda.synchronize()
        res[scatter] = (out.detach().cpu(), dict(zip(L.grad_names(c), [g.detach().cpu() for g in grads])))
    assert len(seen) == 2 and seen[0][0] is None and seen[1][0] and seen[0][1] and seen[1][1], "XF_SCATTER=True did not take the record path"
    assert L.scatter_plan(c)["n_maps"] > 0
    assert torch.equal(res[True][0], res[False][0])
    for scatter in (False, True):
        _gate(c, si, "records" if scatter else "atomics", *res[scatter])
        if c.special == "void-view":                                 # mass 0: nothing reaches the view's maps or reference points
            g = res[scatter][1]
            assert not g["refs"][1].any() and all(not g[f"v1.map{l}"].any() for l in range(c.lp[1][0])), scatter
    if c.special == "void-view":
        _, sv = _direct_forward(c, si, True)
        assert not sv[1, :, 128:136].any() and sv[0, :, 128:136].any(), "the in-bounds mass of the void view"


# ---------------------------------------------------------------------------------------------------------------------
# the two C entries, called as XattnFfnBlocksFn calls them
# ---------------------------------------------------------------------------------------------------------------------
def _tables(c):
    from dpft_amd.models.fusers import train_fused as tf
    layers = _layers(c)
    V = L.n_views(c)
    params = [t for ml in layers for t in tf.view_params(ml)]
    n_levels, n_points = [l for l, _ in c.lp], [p for _, p in c.lp]
    packed, views = tf._pack_views(params, V, n_levels, n_points, torch.device(DEV, 0))
    return dict(V=V, params=params, n_levels=n_levels, n_points=n_points, packed=packed, views=views,
                npts=(C.c_int32 * V)(*n_points))


def _direct_forward(c, si, saved):
    """dpft_xattn_ffn_train_fwd_f32 -> (y3, saved buffer | None) on the CPU."""
    from dpft_amd.hip.lib import Pyramid, lib, make_pyramid, stream
    inp, t = L.cached(c), _tables(c)
    V, B, Q = t["V"], c.B, c.Q
    y1, pos, refs = (inp[k].to(DEV).contiguous() for k in ("y1", "pos", "refs"))
    feats = [[x.to(DEV).contiguous() for x in fv] for fv in inp["feats"]]
    pyrs = (Pyramid * V)(*[make_pyramid(fv) for fv in feats])
    y3 = torch.full_like(y1, float("nan"))
    sv = torch.full((V, B * Q, int(lib.dpft_xattn_ffn_train_saved_floats())), float("nan"), device=DEV) if saved else None
    lib.call("dpft_xattn_ffn_train_fwd_f32", C.cast(pyrs, C.c_void_p), C.cast(t["views"], C.c_void_p), t["packed"].data_ptr(), V,
             C.cast(t["npts"], C.c_void_p), y1.data_ptr(), pos.data_ptr(), refs.data_ptr(), float(c.p_drop), _seed(c, si).data_ptr(),
             int(c.salt), y3.data_ptr(), sv.data_ptr() if saved else None, B, Q, stream())
    torch.cuda.synchronize()
    return y3.cpu(), (sv.cpu() if saved else None)


def _direct(c, si, saved, scratch=False, reps=None):
    """Forward and backward through the C entries -> (y3, {name: gradient}, scratch buffer | None), CPU.  ``saved``: the forward
    keeps the gathered features and the backward reads them (xf_train_bwd_kernel<true>), else both get NULL (<false>);
    ``scratch``: a record buffer, NaN-filled; ``reps``: {(view, level): gradient replicas}, folded with ops.sum_leading."""
    from dpft_amd.hip import ops
    from dpft_amd.hip.lib import Pyramid, lib, make_pyramid, stream
    from dpft_amd.models.fusers import train_fused as tf
    reps = reps or {}
    inp, t = L.cached(c), _tables(c)
    V, B, Q = t["V"], c.B, c.Q
    y1, pos, refs, gy = (inp[k].to(DEV).contiguous() for k in ("y1", "pos", "refs", "gy"))
    feats = [[x.to(DEV).contiguous() for x in fv] for fv in inp["feats"]]
    seed = _seed(c, si)
    pyrs = (Pyramid * V)(*[make_pyramid(fv) for fv in feats])
    y3 = torch.full_like(y1, float("nan"))
    sv = torch.full((V, B * Q, int(lib.dpft_xattn_ffn_train_saved_floats())), float("nan"), device=DEV) if saved else None
    head = (C.cast(t["views"], C.c_void_p), t["packed"].data_ptr(), V, C.cast(t["npts"], C.c_void_p), y1.data_ptr(), pos.data_ptr(),
            refs.data_ptr(), float(c.p_drop), seed.data_ptr(), int(c.salt))
    lib.call("dpft_xattn_ffn_train_fwd_f32", C.cast(pyrs, C.c_void_p), *head, y3.data_ptr(), sv.data_ptr() if saved else None, B, Q, stream())
    gbuf = [[torch.zeros(((reps[(v, l)],) if (v, l) in reps else ()) + tuple(x.shape), device=DEV) for l, x in enumerate(fv)]
            for v, fv in enumerate(feats)]
    gpyr = (Pyramid * V)(*[make_pyramid(fv, gv) for fv, gv in zip(feats, gbuf)])
    assert all(gpyr[v].grad_replicas[l] == r for (v, l), r in reps.items())
    rows = torch.full((V, B * Q, int(lib.dpft_xattn_ffn_train_row_floats())), float("nan"), device=DEV)
    dy1, dqp, dref = (torch.full_like(x, float("nan")) for x in (y1, y1, refs))
    scr = torch.full((V, B * Q, int(lib.dpft_xattn_ffn_train_scratch_floats())), float("nan"), device=DEV) if scratch else None
    lib.call("dpft_xattn_ffn_train_bwd_f32", C.cast(gpyr, C.c_void_p), *head, sv.data_ptr() if saved else None, gy.data_ptr(),
             dy1.data_ptr(), dqp.data_ptr(), dref.data_ptr(), rows.data_ptr(), scr.data_ptr() if scratch else None, B, Q, stream())
    wg = tf._xf_weight_grads(rows, t["n_levels"], t["n_points"])
    grads = {"y1": dy1, "pos": ops.sum_leading([dqp], pos.shape), "refs": dref}
    for v in range(V):
        for l, g in enumerate(gbuf[v]):
            grads[f"v{v}.map{l}"] = ops.sum_leading([g], feats[v][l].shape) if (v, l) in reps else g
    for v in range(V):
        grads.update({f"v{v}.{n}": g for n, g in zip(L.PARAMS, wg[22 * v + 6:22 * v + 22])})
    torch.cuda.synchronize()
    assert list(grads) == L.grad_names(c)
    return y3.cpu(), {k: g.detach().cpu() for k, g in grads.items()}, (scr.cpu() if scratch else None), dqp.cpu()


@pytest.mark.parametrize("name", L.NOSAVE)
def test_backward_without_saved_features(name):
    """saved == NULL: the forward keeps nothing and xf_train_bwd_kernel<false> gathers again.  y3 is the saving forward's bit for
    bit; dy1, dqp (summed to d pos), dref, the maps and `rows` (turned into the parameter gradients by the specs of
    XattnFfnBlocksFn.backward) pass the fp64 gates.  The two instantiations are compiled under different register budgets, so the
    difference from the saved path is printed, not asserted to be zero."""
    c = L.by_name(name)
    for si in range(len(c.seeds)):
        y3, grads, _, dqp = _direct(c, si, saved=False)
        y3s, gs, _, dqps = _direct(c, si, saved=True)
        assert torch.equal(y3, y3s), (name, si)
        assert torch.isfinite(dqp).all()
        diff = {k: float((grads[k] - gs[k]).abs().max()) for k in grads}
        k = max(diff, key=diff.get)
        print(f"XATTN-LATTICE {L.run_id((c, si)):18s} largest |no-save - saved|: {diff[k]:.3e} on {k}; dqp {float((dqp - dqps).abs().max()):.3e}")
        _gate(c, si, "no-save", y3, grads)
        _gate(c, si, "saved", y3s, gs)


def test_replicated_and_recorded_maps_in_one_call():
    """A record buffer and a replicated map in one call (reachable through the C entry only): the 4x4 map with three gradient
    replicas is kept out of the slots and stays on atomics with bq % 3, the plain 8x8 map is recorded (slot 0 of the NaN-filled
    record buffer is written, slots 1-4 are not), the 50x50 map is large.  All three map gradients against fp64."""
    c = L.REPLICATED
    assert L.scatter_plan(c, L.REPLICATED_REPS)["slots"] == [[-1, 0, -1]]
    y3, grads, scr, _ = _direct(c, 0, saved=True, scratch=True, reps=L.REPLICATED_REPS)
    bits, fill = scr.view(torch.int32), int(torch.tensor(float("nan")).view(torch.int32))
    assert torch.isfinite(scr[..., :256]).all() and (bits[..., 256:288] != fill).all(), "the payload and slot 0 of every row are written"
    assert (bits[..., 288:] == fill).all(), "only one map is recorded"
    _gate(c, 0, "rep+records", y3, grads)
    y3a, ga, none, _ = _direct(c, 0, saved=True, scratch=False, reps=L.REPLICATED_REPS)
    assert none is None and torch.equal(y3, y3a)
    _gate(c, 0, "rep+atomics", y3a, ga)
