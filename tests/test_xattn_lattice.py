"""The lattice of the training decoder's cross-attention + FFN block (tests/xattn_lattice.py), checked without a GPU: the table
reaches every item it names (one predicate per item); no sample position lies within 2^-10 pixel of a kink and a float32 replay
keeps every cell, with no row left out; the fp64 reference is O.mlfusion's cross-attention + FFN half; the float32 yardstick of
every tensor is finite and non-zero; the placed values are what they claim; and the two C entries refuse what xf_fill refuses
before anything is launched.  The GPU half is tests/test_gpu_xattn_lattice.py."""
import ctypes as C

import pytest
import torch

from tests import xattn_lattice as L

A = L.A


def _plan(name):
    return L.scatter_plan(L.by_name(name))


def _px(c):
    return [[h * w for h, w in maps] for maps in c.maps]


# one predicate per item of the module's list; each names the case(s) that reach it
ITEMS = {
    1: lambda: any(L.n_views(c) == 4 and c.p_drop > 0 for c in L.CASES) and any(L.n_views(c) == 4 and c.p_drop == 0 for c in L.CASES),
    2: lambda: any(len(set(c.lp)) == L.n_views(c) >= 4 for c in L.CASES) and any(len({p for _, p in c.lp}) > 1 for c in L.CASES)
    and any(len({l for l, _ in c.lp}) > 1 for c in L.CASES),
    3: lambda: any(l == 8 and p == 2 and sorted(px)[L.MAX_SLOTS - 1] == sorted(px)[L.MAX_SLOTS] and max(px) <= L.REC_PIXELS
                   and sorted(s for s in plan if s >= 0) == list(range(L.MAX_SLOTS)) and plan.count(-1) == 3
                   for c in L.CASES for (l, p), px, plan in zip(c.lp, _px(c), L.scatter_plan(c)["slots"])),
    4: lambda: {c.name for c in L.CASES} >= set(L.NOSAVE) and any(L.by_name(n).p_drop > 0 for n in L.NOSAVE)
    and any(L.n_views(L.by_name(n)) == 4 for n in L.NOSAVE),
    5: lambda: any(c.B > 1 and c.Q % 4 and (c.B * c.Q) % 4 for c in L.CASES) and any(c.Q == 1 and c.B == 1 for c in L.CASES)
    and any(c.Q == 1 and c.B > 1 for c in L.CASES) and any(c.B * c.Q > 2 * L.REPLICAS and L.replicated_levels(c) for c in L.CASES),
    6: lambda: _plan("one-row")["nchunk0"] == 8 > L.by_name("one-row").Q and _plan("one-row")["nchunk"] == 1
    and _plan("chunks-4")["nchunk0"] == 4 == _plan("chunks-4")["nchunk"] and _plan("chunks-4")["last"] == 1
    and _plan("limit-2048")["qchunk"] == 2 and _plan("limit-2048")["last"] == 1 and _plan("limit-2048")["nchunk"] == 5,
    7: lambda: any(2048 in px and 2049 in px and plan[px.index(2048)] >= 0 and plan[px.index(2049)] == -1
                   for c in L.CASES for px, plan in zip(_px(c), L.scatter_plan(c)["slots"]))
    and any(256 in px and 257 in px for c in L.CASES for px in _px(c))
    and L.scatter_plan(L.REPLICATED, L.REPLICATED_REPS)["slots"] == [[-1, 0, -1]],
    8: lambda: len(L.PARAMS) == 16 and all(n in L.grad_names(c) for c in L.CASES for n in ("y1", "pos", "refs")),
    9: lambda: {c.special for c in L.CASES} >= {"mish-sat", "flat-ln2", "void-view", "softmax-120"},
    10: lambda: len(REFUSALS) >= 7,
}


def test_table_reaches_every_item():
    print("\n".join(L.table_rows()))
    assert len({c.name for c in L.CASES}) == len(L.CASES) == 12
    for c in L.CASES + [L.REPLICATED]:
        assert c.B * c.Q <= 160 and len(c.maps) == L.n_views(c) <= 4 and c.why, c.name
        assert all(len(m) == l and 1 <= p <= 4 and l * p <= 20 and l <= 8 for (l, p), m in zip(c.lp, c.maps)), c.name
        small = all(h <= 64 and w <= 64 and h * w <= 64 * 40 for m in c.maps for h, w in m)
        assert small or c.name in ("wrap-replicas", "limit-2048"), c.name           # where a limit needs more
    for item, pred in ITEMS.items():
        assert pred(), f"item {item} is not reached"
        assert item == 10 or any(item in L.items_of(c) for c in L.CASES + [L.REPLICATED]), f"no case's why names item {item}"
    # the record plan of the eight-map view: the 24-pixel tie is cut between levels 2 and 4
    assert L.scatter_plan(L.by_name("v4-mixed"))["slots"][2] == [3, -1, 4, 2, -1, 1, -1, 0]
    assert all(isinstance(s, int) and -2 ** 63 <= s < 2 ** 63 for c in L.CASES for s in c.seeds)
    d4 = L.by_name("dropout-v4")
    assert d4.seeds[0] >> 32 and d4.seeds[1] < 0 and d4.salt == 9 and d4.p_drop == 0.25 and L.by_name("dropout-odd").p_drop == 0.5


@pytest.mark.parametrize("c", L.CASES + [L.REPLICATED], ids=lambda c: c.name)
def test_no_kinks_and_the_float32_replay_keeps_every_cell(c):
    a, b = L.make_inputs(c), L.make_inputs(c)
    assert torch.equal(a["refs"], b["refs"]) and all(torch.equal(x, y) for p, q in zip(a["params"], b["params"])
                                                     for x, y in zip(p.values(), q.values())), c.name
    fig = L.check_inputs(c)
    print(c.name, fig)
    assert fig["rows_dropped"] == 0 and fig["replay"] <= L.REPLAY == 2.0 ** -16
    assert 0.02 <= fig["outside"] <= (0.6 if c.special == "void-view" else 0.35), (c.name, fig["outside"])


def test_reference_is_the_second_half_of_mlfusion():
    """O.mlfusion with a self-attention that adds nothing (out_proj = 0) and norm1 = identity on an already normalised query is
    LN(query) followed by the cross-attention + FFN half: the lattice's ``block`` on y1 = LN(query), p = 0."""
    from oracle import dprt_oracle as O
    c = L.by_name("v4-mixed")
    inp = L.cached(c)
    for v, (nl, P) in enumerate(c.lp):
        sd = {"ml." + k: t.double() for k, t in inp["params"][v].items()}
        g = torch.Generator().manual_seed(v)
        sd.update({"ml.self_attn.in_proj_weight": torch.randn(48, 16, generator=g, dtype=torch.float64),
                   "ml.self_attn.in_proj_bias": torch.randn(48, generator=g, dtype=torch.float64),
                   "ml.self_attn.out_proj.weight": torch.zeros(16, 16, dtype=torch.float64),
                   "ml.self_attn.out_proj.bias": torch.zeros(16, dtype=torch.float64),
                   "ml.norm1.weight": torch.ones(16, dtype=torch.float64), "ml.norm1.bias": torch.zeros(16, dtype=torch.float64)})
        query, pos = inp["y1"][v].double(), inp["pos"].double()
        levels = [t.double() for t in inp["feats"][v]]
        want = O.mlfusion(query, levels, inp["refs"][v].double(), pos.unsqueeze(0), sd, "ml", 8, P)
        got = L.block(P, O._ln(query, sd, "ml.norm1"), pos, inp["refs"][v].double(), levels, sd)
        assert float((got - want).abs().max()) <= 1e-12, (v, float((got - want).abs().max()))


@pytest.mark.parametrize("run", L.RUNS + [(L.REPLICATED, 0)], ids=L.run_id)
def test_fp32_yardstick_is_finite_and_non_zero(run):
    c, si = run
    r64, r32 = L.cached_reference(c, torch.float64, si), L.cached_reference(c, torch.float32, si)
    assert torch.isfinite(r64["y3"]).all() and torch.isfinite(r32["y3"]).all()
    d = {"y3": float((r32["y3"].double() - r64["y3"]).abs().max())}
    zero = set()
    for n in L.grad_names(c):
        a, b = r64["grads"][n], r32["grads"][n]
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), (c.name, n)
        d[n] = float((b.double() - a).abs().max())
        if not a.any():
            zero.add(n)
            assert not b.any(), (c.name, n)
    print(c.name, {k: f"{v:.2e}" for k, v in d.items()})
    assert zero == L.expected_zero(c), (c.name, zero ^ L.expected_zero(c))
    for n, v in d.items():
        assert (v == 0) if n in zero | L.expected_exact(c) else (0 < v < float("inf")), (c.name, n, v)
    # the yardstick of y3 stays inside the forward rule: a failure on the GPU is the kernel's
    assert L.distance(r32["y3"], r64["y3"]) <= 1.0, (c.name, L.distance(r32["y3"], r64["y3"]))


def test_placed_values_are_what_they_claim():
    import torch.nn.functional as F
    from oracle import dprt_oracle as O
    # mish-sat: every pre-activation within 0.1 of its placed value, both sides of the x > 20 switch and of expf's overflow
    c = L.by_name("mish-sat")
    inp = L.cached(c)
    for dt in (torch.float64, torch.float32):
        sd = {"ml." + k: t.to(dt) for k, t in inp["params"][0].items()}
        y1, pos = inp["y1"][0].to(dt), inp["pos"].to(dt)
        ca = O.ms_deform_attn(y1 + pos.unsqueeze(0), inp["refs"][0].to(dt), [t.to(dt) for t in inp["feats"][0]], sd,
                              "ml.ms_deform_attn", 8, c.lp[0][1], core=O.msda_core_floor)
        pre = F.linear(O._ln(y1 + ca, sd, "ml.norm2"), sd["ml.ffn1.weight"], sd["ml.ffn1.bias"])
        placed = torch.tensor(L.MISH_PLACED, dtype=dt)
        assert float((pre - placed).abs().max()) < 0.1, float((pre - placed).abs().max())
    assert len(L.MISH_PLACED) == 32 and set(L.MISH_PLACED) >= {s * x for s in (1, -1) for x in (100, 60, 25, 20.5, 20, 19.5, 1, 0, 89, 104)}
    assert ((pre > 20) & (pre < 21)).any() and ((pre <= 20) & (pre > 19)).any() and (pre > 88.73).any() and (pre < -88.73).any()
    # flat-ln2: the rows of view 1 are constant, on the grid, and the attention adds exactly nothing -> variance exactly 0
    c = L.by_name("flat-ln2")
    inp = L.cached(c)
    y = inp["y1"][1]
    assert torch.equal(y, y[..., :1].expand_as(y)) and torch.equal(y * 64, torch.round(y * 64)) and y.abs().max() > 0
    assert not inp["params"][1][A + "output_proj.weight"].any() and not inp["params"][1][A + "output_proj.bias"].any()
    for dt in (torch.float64, torch.float32):
        assert float(y.to(dt).var(-1, unbiased=False).abs().max()) == 0.0
    assert float(inp["y1"][0].var(-1).min()) > 0 and inp["params"][0][A + "output_proj.weight"].any()
    # void-view: every sample of view 1 outside (mass 0) in fp64 and in the float32 replay; view 0 ordinary
    c = L.by_name("void-view")
    inp = L.cached(c)
    p = inp["params"][1]
    assert not p[A + "sampling_offsets.weight"].any() and max(w for _, w in c.maps[1]) <= 32
    assert torch.equal(p[A + "sampling_offsets.bias"].view(8, 3, 4, 2)[..., 0], torch.full((8, 3, 4), 64.0))
    for dt in (torch.float64, torch.float32):
        t = L.positions(inp["refs"][1].to(dt), L.offsets(inp["y1"][1].to(dt), inp["pos"].to(dt), p, 3, 4), c.maps[1])
        assert not L.inside(t, c.maps[1]).any()
    r64 = L.cached_reference(c)
    assert not r64["grads"]["refs"][1].any() and r64["grads"]["refs"][0].any()
    # softmax-120: the bias alternates +-60
    b = L.cached(L.by_name("softmax-120"))["params"][0][A + "attention_weights.bias"]
    assert torch.equal(b[0::2], torch.full_like(b[0::2], 60.0)) and torch.equal(b[1::2], torch.full_like(b[1::2], -60.0))


# ---------------------------------------------------------------------------------------------------------------------
# item 10: the entries' refusals
# ---------------------------------------------------------------------------------------------------------------------
REFUSALS = [
    ("V = 5", dict(V=5), b"bad sizes (V=5"),
    ("V = 0", dict(V=0), b"bad sizes (V=0"),
    ("P = 5", dict(P=5), b"L=2, P=5 exceed"),
    ("L P = 21", dict(L=7, P=3), b"L=7, P=3 exceed"),
    ("L = 9", dict(L=9, P=1), b"L=9, P=1 exceed"),
    ("p_drop = 1", dict(p=1.0), b"dropout probability"),
    ("p_drop < 0", dict(p=-0.25), b"dropout probability"),
    ("B = 0", dict(B=0), b"bad sizes"),
] + [(f"null {n}", dict(null=n), b"null argument") for n in ("pyr", "views", "packed", "n_points", "y1", "pos", "ref", "seed")]


def _entry_args(V=1, L=2, P=2, p=0.0, B=1, Q=1, null=None, no_grad_level=None):
    from dpft_amd.hip.lib import DecoderView, Pyramid
    pyr = (Pyramid * 4)()
    for v in range(4):
        pyr[v].L = L
        for l in range(min(L, 8)):
            pyr[v].level[l], pyr[v].grad[l], pyr[v].H[l], pyr[v].W[l] = 4096 * (l + 1), 8192 * (l + 1), 4, 4
    if no_grad_level is not None:
        pyr[0].grad[no_grad_level] = None
    views, npts = (DecoderView * 4)(), (C.c_int32 * 4)(P, P, P, P)
    keep = (pyr, views, npts)
    a = dict(pyr=C.cast(pyr, C.c_void_p), views=C.cast(views, C.c_void_p), packed=C.c_void_p(1 << 20), V=V,
             n_points=C.cast(npts, C.c_void_p), y1=C.c_void_p(2 << 20), pos=C.c_void_p(3 << 20), ref=C.c_void_p(4 << 20), p=p,
             seed=C.c_void_p(5 << 20), salt=1)
    if null:
        a[null] = None
    return keep, list(a.values()), B, Q


def test_entries_refuse_what_xf_fill_refuses():
    """dpft_xattn_ffn_train_fwd_f32 / _bwd_f32: DPFT_ERR_ARG (-1) with a message that names xattn_ffn_train, returned by xf_fill
    and the null checks behind it before any launch (the device pointers are never read; a launch without a device would come
    back as another code)."""
    from dpft_amd.hip.lib import lib
    err = lambda: lib.dpft_last_error()       # noqa: E731
    out = [C.c_void_p((6 + i) << 20) for i in range(8)]

    def fwd(kw, y3=out[0]):
        keep, a, B, Q = _entry_args(**kw)
        return lib.dpft_xattn_ffn_train_fwd_f32(*a, y3, out[1], B, Q, None)

    def bwd(kw, outs=None):
        keep, a, B, Q = _entry_args(**kw)
        o = list(out[2:7]) if outs is None else outs
        return lib.dpft_xattn_ffn_train_bwd_f32(*a, out[1], *o, None, B, Q, None)
    for what, kw, msg in REFUSALS:
        for fn in (fwd, bwd):
            assert fn(kw) == -1 and b"xattn_ffn_train" in err() and msg in err(), (what, fn.__name__, err())
    assert fwd({}, y3=None) == -1 and b"xattn_ffn_train_fwd: null output" in err()
    for i in range(5):                                               # dy3, dy1, dqp, dref, rows
        o = list(out[2:7])
        o[i] = None
        assert bwd({}, o) == -1 and b"xattn_ffn_train_bwd: null argument" in err(), i
    for level in (0, 1):
        assert bwd(dict(no_grad_level=level)) == -1 and b"xattn_ffn_train: view 0 level %d has no gradient buffer" % level in err()
    keep, a, B, Q = _entry_args()
    keep[0][0].level[1] = None
    assert lib.dpft_xattn_ffn_train_fwd_f32(*a, out[0], out[1], B, Q, None) == -1 and b"xattn_ffn_train: view 0 level 1 is invalid" in err()
