"""The training decoder's view reduction + detection head + reference points (dpft_amd/csrc/decoder_train_h.hip through
train_fused.head_block, reference_points and RefPointsFn) against the fp64 oracle over the lattice of tests/head_lattice.py: V = 1..4,
1 / 2 / 15 / 16 classes, every row remainder of the four-wave block, a different T, P and (H, W) per (batch element, view), 3- and
4-row projections, every shape form, and reference-point rows placed on the clip edges, at w == 0, at the origin, on the vertical
axis, on the +-180 degree cut and at elevations up to 89.99 degrees.  The CPU half (tests/test_head_lattice.py) shows that every
case reaches its rows and that its inputs let no error hide.

The rule is the one of the decoder lattice, elementwise |got - ref| <= 1e-4 |ref| + 1e-5 max|ref|, written as a distance <= 1, on
every output and on every gradient element by element (dy3, d prev_center, the 13 weight gradients).  A tensor that misses it
may pass on 4x the distance of the fp32 yardstick for that tensor: the oracle evaluated in float32, with the closed form in
float32 on the rows at 89 degrees or more and on the axis (where fp32 autograd has no digits left or is NaN).  Nothing is
measured against the kernel's own output.  Every distance is printed (``HEAD-LATTICE`` lines)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import head_lattice as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


_MODULES = {}


def _modules(c, inp):
    """The case's layer and head on the device, built once (the weights are never changed)."""
    if c.name not in _MODULES:
        _MODULES[c.name] = _build_modules(c, inp)
    return _MODULES[c.name]


def _build_modules(c, inp):
    from dpft_amd.models.fusers.mpfusion import MPFusion
    from dpft_amd.models.heads.detection import LinearDetectionHead
    V = L.n_views(c)
    layer = MPFusion(V, d_model=16, d_ffn=32, n_levels=[2] * V, n_heads=[8] * V, n_points=[2] * V, activation="Mish", norm=True,
                     reduction="linear").to(DEV)
    head = LinearDetectionHead(16, c.ncls, 3, 3).to(DEV)
    from dpft_amd.models.fusers import train_fused as tf
    assert tf.head_supported(layer, head)
    with torch.no_grad():
        for p, w in zip(tf.head_params(layer, head), inp["weights"]):
            assert p.shape == w.shape
            p.copy_(w)
    return layer, head


def _proj(inp, perm=None):
    from dpft_amd.models.fusers import train_fused as tf
    pick = (lambda t: t) if perm is None else (lambda t: t[perm].contiguous())
    return tf._Proj([(pick(T).to(DEV), pick(P).to(DEV)) for T, P in zip(inp["T"], inp["P"])],
                    [pick(s).to(DEV) for s in inp["shape"]], inp["flags"])


def _run(c, present=L.ALL, want_refs=True, perm=None):
    """head_block forward + backward from the cotangents named in ``present`` -> (outs [6] (refs None without), grads [15]), CPU."""
    from dpft_amd.models.fusers import train_fused as tf
    inp = L.cached(c)["inp"]
    layer, head = _modules(c, inp)
    pb = (lambda t: t) if perm is None else (lambda t: t[perm].contiguous())
    pv = (lambda t: t) if perm is None else (lambda t: t[:, perm].contiguous())
    y3 = pv(inp["y3"]).to(DEV).requires_grad_(True)
    prev = pb(inp["prev"]).to(DEV).requires_grad_(True)
    gys = [pb(g) for g in inp["gys"][:5]] + [pv(inp["gys"][5])]
    weights = tf.head_params(layer, head)
    x, out, refs = tf.head_block(layer, head, _proj(inp, perm), y3, prev, want_refs)
    outs = [x, out["center"], out["size"], out["angle"], out["class"], refs]
    assert (refs is not None) == want_refs
    sel = [(o, g.to(DEV)) for n, o, g in zip(L.OUT_NAMES, outs, gys) if n in present and o is not None]
    grads = torch.autograd.grad([o for o, _ in sel], [y3, prev] + weights, [g for _, g in sel], allow_unused=True)
    torch.cuda.synchronize()
    assert all(g is not None for g in grads)
    return [None if o is None else o.detach().cpu() for o in outs], [g.detach().cpu() for g in grads]


_RUNS = {}


def _full_run(c):
    if c.name not in _RUNS:
        _RUNS[c.name] = _run(c)
    return _RUNS[c.name]


def _assert_rule(c, tag, names, got, ref64, ref32):
    """Every tensor under the fixed rule, or under 4x its fp32 yardstick's distance; ``ref32`` is called only when needed."""
    worst, rule, y32 = 0.0, "fixed", None
    for i, (n, a, r) in enumerate(zip(names, got, ref64)):
        if a is None:
            continue
        assert a.shape == r.shape and torch.isfinite(a).all(), (c.name, tag, n, "shape / NaN / Inf")
        d = L.distance(a, r)
        if d > 1.0:
            y32 = ref32() if y32 is None else y32
            d32 = L.distance(y32[i], r)
            print(f"HEAD-LATTICE {c.name:11s} {tag:14s} {n:10s} distance {d:10.4f}   fp32 yardstick {d32:8.4f}")
            assert d <= 4.0 * d32, (c.name, tag, n, d, d32)
            rule = "4x fp32"
        worst = max(worst, d)
    print(f"HEAD-LATTICE {c.name:11s} {tag:14s} worst distance {worst:8.4f}  rule {rule}")


def _check(c, tag, outs, grads, present, want_refs=True):
    key = present if want_refs else present - {"refs"}
    ref64 = L.cached_reference(c, torch.float64, key)
    ref32 = lambda: L.cached_reference(c, torch.float32, key)       # noqa: E731
    _assert_rule(c, tag + " out", L.OUT_NAMES, outs, ref64["outs"], lambda: ref32()["outs"])
    _assert_rule(c, tag + " grad", L.GRAD_NAMES, grads, ref64["grads"], lambda: ref32()["grads"])


@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_forward_and_backward_match_fp64_oracle(c):
    """head_block(..., want_refs=True): x, center, size, angle, class, refs and dy3, d prev_center and the 13 weight gradients,
    element by element.  The steep cases fail here on the ill-conditioned form of the elevation's gradient
    (asin'(tz / r) d(tz / r): at 89.99 degrees the distance is ~1e15)."""
    outs, grads = _full_run(c)
    _check(c, "refs", outs, grads, L.ALL)


@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_without_reference_points(c):
    outs, grads = _run(c, L.ALL - {"refs"}, want_refs=False)
    assert outs[5] is None
    _check(c, "no-refs", outs, grads, L.ALL, want_refs=False)
    full = _full_run(c)[0]
    assert all(torch.equal(a, b) for a, b in zip(outs[:5], full[:5])), c.name


@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_null_gradient_inputs(c):
    """Each of the backward's six gradient inputs absent in turn, and all of them but one."""
    for n in L.OUT_NAMES:
        for present in (L.ALL - {n}, frozenset({n})):
            outs, grads = _run(c, present)
            tag = ("-" + n) if len(present) > 1 else ("only " + n)
            key = frozenset(present)
            ref64 = L.cached_reference(c, torch.float64, key)
            _assert_rule(c, tag, L.GRAD_NAMES, grads, ref64["grads"], lambda: L.cached_reference(c, torch.float32, key)["grads"])


@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_second_launch_is_bit_equal(c):
    """No atomics anywhere in the block (the weight gradients are fixed-order row sums): a second run repeats every bit."""
    outs, grads = _full_run(c)
    outs2, grads2 = _run(c)
    for n, a, b in zip(L.OUT_NAMES + L.GRAD_NAMES, outs + grads, outs2 + grads2):
        assert torch.equal(a, b), (c.name, n)


EXACT = [c for c in L.CASES if c.exact]


@pytest.mark.parametrize("c", EXACT, ids=L.case_id)
def test_reference_point_entries_are_bit_equal_to_the_head_block(c):
    """Where the centre branch adds exactly zero (center == prev_center): reference_points(proj, center) is the head block's refs
    bit for bit, and RefPointsFn's backward (ref_points_bwd_kernel) is the head backward's dcenter_prev when only drefs is given
    -- the same ref_point<true> per view and the same order of the view sum."""
    from dpft_amd.models.fusers import train_fused as tf
    inp = L.cached(c)["inp"]
    outs, _ = _full_run(c)
    assert torch.equal(outs[1], inp["prev"]), c.name
    proj = _proj(inp)
    prev = inp["prev"].to(DEV)
    assert torch.equal(tf.reference_points(proj, prev).cpu(), outs[5]), c.name
    _, grads = _run(c, frozenset({"refs"}))
    leaf = prev.clone().requires_grad_(True)
    refs = tf.RefPointsFn.apply(proj, leaf)
    assert torch.equal(refs.detach().cpu(), outs[5])
    (dc,) = torch.autograd.grad(refs, leaf, inp["gys"][5].to(DEV))
    assert torch.equal(dc.cpu(), grads[1]), (c.name, float((dc.cpu() - grads[1]).abs().max()))
    # and against the reference: the closed form on the axis and the steep rows, the oracle's autograd elsewhere
    key = frozenset({"refs"})
    _assert_rule(c, "RefPointsFn", ("prev",), [dc.cpu()], [L.cached_reference(c, torch.float64, key)["grads"][1]],
                 lambda: [L.cached_reference(c, torch.float32, key)["grads"][1]])


@pytest.mark.parametrize("name", ["v4-c16", "v1-c1"])
def test_pack_head_layout(name):
    """dpft_decoder_pack_head_f32 against the layout of decoder_pack.h restated in numpy: PH_RED_WT [v 4][k 16][o 16] =
    reduction_layer.weight[o][k * V + v] (views >= V zero), PH_W [layer 3][k 16][branch 4][o 16] = W[branch][layer][o][k] (rows
    >= out_features zero)."""
    from dpft_amd.hip.lib import lib, stream
    c = L.by_name(name)
    V, w = L.n_views(c), [t.numpy() for t in L.cached(c)["inp"]["weights"]]
    want = np.zeros(4 * 256 + 3 * 1024, np.float32)
    red = want[:1024].reshape(4, 16, 16)
    for v in range(V):
        red[v] = w[0].reshape(16, 16, V)[:, :, v].T
    hw = want[1024:].reshape(3, 16, 4, 16)
    for g in range(4):
        for layer in range(3):
            m = w[1 + 3 * g + layer]
            hw[layer, :, g, :m.shape[0]] = m.T
    assert int(lib.dpft_decoder_packed_head_floats()) == want.size
    dev = [t.to(DEV).contiguous() for t in L.cached(c)["inp"]["weights"]]
    packed = torch.full((want.size,), float("nan"), device=DEV)
    ptrs = (C.c_void_p * 12)(*[t.data_ptr() for t in dev[1:]])
    lib.call("dpft_decoder_pack_head_f32", dev[0].data_ptr(), C.byref(ptrs), V, c.ncls, packed.data_ptr(), stream())
    torch.cuda.synchronize()
    assert np.array_equal(packed.cpu().numpy(), want), name


@pytest.mark.parametrize("name,perm", [("v4-c16", [2, 0, 1]), ("poles", [1, 0]), ("generic-v3", [1, 0])])
def test_batch_permutation_permutes_and_changes_nothing_else(name, perm):
    """T, P, the shape rows, y3, prev_center and the cotangents of the batch elements permuted together: the outputs, dy3 and
    d prev_center are the permuted ones bit for bit (a row's result depends on its own batch element's matrices alone); the
    weight gradients sum the same rows in another order and stay under the rule."""
    c = L.by_name(name)
    assert sorted(perm) == list(range(c.B)) and perm != list(range(c.B))
    outs, grads = _full_run(c)
    pouts, pgrads = _run(c, perm=perm)
    for n, a, b in zip(L.OUT_NAMES[:5], outs[:5], pouts[:5]):
        assert torch.equal(a[perm], b), (name, n)
    assert torch.equal(outs[5][:, perm], pouts[5]) and torch.equal(grads[0][:, perm], pgrads[0]) and torch.equal(grads[1][perm], pgrads[1])
    ref64 = L.cached_reference(c)
    _assert_rule(c, "permuted", L.GRAD_NAMES[2:], pgrads[2:], ref64["grads"][2:], lambda: L.cached_reference(c, torch.float32)["grads"][2:])
