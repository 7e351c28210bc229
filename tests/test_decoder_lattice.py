"""The geometry lattice of the fused inference decoder (tests/decoder_lattice.py), checked without a GPU: every case reaches the edge
it is there for (its arithmetic against the limits the library reports, dpft_decoder_limits: host code), its seeded inputs make
the comparison mean something, fused.supported() follows the library's limit, and the fp32 evaluation of the oracle stays within a
quarter of the tolerance of its fp64 value, so that the rule has room and a failure on the GPU is the kernel's.  The GPU half is
tests/test_gpu_decoder_lattice.py."""
import ctypes as C
import math

import pytest
import torch

from tests import decoder_lattice as L


def test_limits_are_exported():
    from dpft_amd.hip.lib import lib
    QC, NS, XR, QMAX = L.limits()
    assert QC >= 2 and QC % 2 == 0 and NS >= 2 and XR >= 1
    # the largest admitted Q is the score kernel's 62 KiB of LDS: K/V rows with one pad per slice, maxima, query rows, partials
    lds = lambda Q: 4 * (4 * (Q + NS) + 16 + 2 * QC + 4 * QC * NS)
    assert lds(QMAX) <= 62 * 1024 < lds(QMAX + 1)
    assert lib.dpft_decoder_limits(None) == -1 and b"decoder_limits: null output" in lib.dpft_last_error()
    # the entry points refuse a larger Q with a message that names the limit, before they touch a pointer's target
    one = C.c_void_p(64)
    assert lib.dpft_decoder_attn0_f32(one, one, QMAX + 1, 1, one, None) == -1
    msg = lib.dpft_last_error().decode()
    assert f"{QMAX + 1} queries do not fit" in msg and f"at most {QMAX}" in msg
    from dpft_amd.hip.lib import DecoderFwd
    d = DecoderFwd()
    d.B, d.Q, d.V, d.iters, d.num_classes = 1, QMAX + 1, 1, 1, 2
    for field in ("packed_views", "packed_heads", "pyr", "query0", "pos", "center0", "work", "center", "size", "angle", "cls"):
        setattr(d, field, 64)
    assert lib.dpft_decoder_forward_f32(C.byref(d), None) == -1
    msg = lib.dpft_last_error().decode()
    assert f"{QMAX + 1} queries do not fit" in msg and f"at most {QMAX}" in msg
    print("\n".join(L.table_rows()))


def test_table_reaches_what_it_claims():
    QC, NS, XR, QMAX = L.limits()
    c = {x.name: x for x in L.CASES}
    assert len(c) == len(L.CASES)
    BQ = lambda x: x.B * x.Q
    V = L.n_views
    for x in L.CASES:
        assert 1 <= x.Q <= QMAX and 1 <= V(x) <= 4 and 1 <= x.ncls <= 16 and 1 <= x.iters <= 8, x.name
        assert all(1 <= l <= len(L.LEVELS) and 1 <= p <= 4 and l * p <= 20 for l, p in x.LP), x.name
    # anchor: the product's slot table (all 160 slots live) and iteration count off Q = 400, with both row tails
    a = c["anchor"]
    assert a.Q != 400 and all(l * p == 20 for l, p in a.LP) and V(a) == 3 and a.iters == 4 and a.ncls == 2
    assert BQ(a) % XR == 4 and a.Q % QC == 0 and a.Q // QC > 1
    # q1: one key; every slice but one empty; the pair partner clipped; one live wave of XR, one head row of 4
    q1 = c["q1"]
    assert q1.Q == 1 and q1.B == 1 and NS - math.ceil(q1.Q / math.ceil(q1.Q / NS)) == NS - 1 and q1.ncls == 1 and q1.LP == ((1, 1),)
    assert BQ(q1) % XR == 1 and BQ(q1) % 4 == 1 and q1.iters == 2
    # below-slices: fewer keys than slices, four views with mixed slot counts, one iteration, 16 classes
    bs = c["below-slices"]
    assert 1 < bs.Q < NS and V(bs) == 4 and bs.iters == 1 and bs.ncls == 16
    assert len({l * p for l, p in bs.LP}) >= 3 and max(l * p for l, p in bs.LP) == 20 and min(l * p for l, p in bs.LP) == 1
    assert {p for _, p in bs.LP} == {1, 2, 3, 4} and len({l for l, _ in bs.LP}) == 4
    assert BQ(bs) % XR == 0 and BQ(bs) % 4 == 1
    sizes = [L.LEVELS[l] for l in range(bs.LP[0][0])]
    assert (1, 1) in sizes and any(h > 1 and w == 1 for h, w in sizes) and any(h == 1 and w > 1 for h, w in sizes)
    # the chunk edge: QC - 1 (odd: the last pair's partner is clipped), QC, QC + 1 (a last chunk of one query); iters = 2
    assert [c[n].Q for n in ("chunk-49", "chunk-50", "chunk-51")] == [QC - 1, QC, QC + 1]
    assert all(c[n].iters == 2 and c[n].LP == ((2, 2), (4, 1)) for n in ("chunk-49", "chunk-50", "chunk-51"))
    # odd-101: odd Q over more than one chunk, both row tails, three-point slots
    o = c["odd-101"]
    assert o.Q % 2 == 1 and o.Q % QC == 1 and BQ(o) % XR == 6 and BQ(o) % 4 == 2 and 3 in {p for _, p in o.LP} and o.iters == 3
    assert all(l * p < 20 for l, p in o.LP) and o.ncls == 3
    # batch-5: the first layer's scores for one batch element against five later on
    assert c["batch-5"].B == 5 and V(c["batch-5"]) == 1 and BQ(c["batch-5"]) % XR == 5 and BQ(c["batch-5"]) % 4 == 2
    # the staging trips of a score block: STAGING items = keys + the chunk's queries
    assert c["q462"].Q + QC == L.STAGING                                   # the last Q of one trip
    assert c["q463"].Q + QC == L.STAGING + 1 and V(c["q463"]) == 2          # one item (a query row) in the second trip
    assert c["q512"].Q == L.STAGING                                        # every query row in the second trip
    assert 2 * L.STAGING < c["q1000"].Q + QC <= 3 * L.STAGING and c["q1000"].Q < QMAX
    assert all(c[n].iters == 2 for n in ("q462", "q463", "q512", "q1000"))  # packed rows and composed rows
    # the score cases: more than one chunk, a slice boundary inside the chunk; packed + composed vs packed only
    u, s = c["scores-uniform"], c["scores-split"]
    assert u.iters == 2 and V(u) == 2 and u.B == 2 and u.Q > QC and s.iters == 1 and s.Q > QC
    SL = math.ceil(s.Q / NS)
    assert L.SPLIT_AT % 2 == 1 and L.SPLIT_AT % SL != 0 and 0 < L.SPLIT_AT < QC       # a pair and a slice straddle the split
    f = c["forms"]
    assert V(f) == 3 and f.special == "clamped" and BQ(f) % XR == 4 and BQ(f) % 4 == 2 and set(L.KINDS[:3]) == {"plain", "transformed", "perspective"}
    assert c["w-zero"].iters == 1 and c["w-zero"].special == "wzero"
    # over the whole table
    assert {x.iters for x in L.CASES} >= {1, 2, 3, 4} and {x.ncls for x in L.CASES} >= {1, 2, 3, 16}
    assert {V(x) for x in L.CASES} == {1, 2, 3, 4}
    assert {BQ(x) % XR for x in L.CASES} >= {0, 1, 2, 4, 5, 6}
    assert {BQ(x) % 4 for x in L.CASES} == {0, 1, 2, 3}
    assert {p for x in L.CASES for _, p in x.LP} == {1, 2, 3, 4}


@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_inputs_make_the_comparison_mean_something(c):
    fuser, inp, out64, trace, out32, a64, a32 = L.cached(c)
    fig = L.check_inputs(c, out64, trace)
    print(c.name, fig)
    assert a64.shape == (L.n_views(c), c.Q, 16) and float(a64.abs().max()) >= 0.1
    for k, n in zip(L.KEYS, (3, 3, 2, c.ncls)):
        assert out64[k].shape == (c.B, c.Q, n) and out64[k].dtype == torch.float64
    if c.special == "wzero":
        T, P = inp["projection"][0]
        w = torch.einsum("bj,bkj->bk", P[:, 2, :3], inp["center0"]) + P[:, 2, 3:4]
        assert 0 < int((w == 0).sum()) < w.numel() and P[0, 2].tolist() == [0.0, 0.0, 1.0, 0.0]
        assert (inp["center0"][..., 2][w == 0] == 0).all()
    if c.name == "forms":
        assert inp["flags"] == [False, True, False]
        assert not inp["projection"][0][0].any() and inp["projection"][1][0].any()      # an all-zero T under "left to the device"


@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_fp32_oracle_is_within_a_quarter_of_the_tolerance(c):
    """The yardstick: the same oracle evaluated in fp32 on the CPU, as a fraction of the tolerance rtol |ref| + 1e-5 max|ref|."""
    fuser, inp, out64, trace, out32, a64, a32 = L.cached(c)
    d = {k: L.distance(out32[k], out64[k]) for k in L.KEYS}
    d["attn0"] = L.distance(a32, a64)
    print(c.name, {k: round(v, 4) for k, v in d.items()})
    for k, v in d.items():
        assert v <= 0.25, (c.name, k, v)


def test_score_cases_take_the_fallback_where_they_mean_to():
    QC, NS, XR, QMAX = L.limits()
    h = L.FALLBACK_HEAD
    # scores-uniform: every slice of the bent head lies more than 100 below its bound, in every layer and view (the rows do not
    # depend on the layer's input: their weights are zero), the other heads nowhere; the exact soft-max is uniform
    c = L.by_name("scores-uniform")
    fuser = L.cached(c)[0]
    for it in range(c.iters):
        for ml in fuser.mpfusion[f"fusion{it}"].ml_fusion_layers.values():
            w = ml.self_attn.in_proj_weight
            assert not w[2 * h:2 * h + 2].any() and not w[16 + 2 * h:16 + 2 * h + 2].any()
        q, k = L.qk_rows(fuser, it, x=torch.randn(c.Q, 16, generator=torch.Generator().manual_seed(it)))
        den = L.slice_log2_den(q, k, NS)                       # (V,8,Q,NS)
        assert not den.isnan().any()
        assert float(den[:, h].max()) < -300, float(den[:, h].max())
        others = [m for m in range(8) if m != h]
        assert float(den[:, others].min()) > -50, float(den[:, others].min())
        s = q[:, h] @ k[:, h].transpose(-1, -2)
        assert float(s.max()) < -160 and float((q[:, h].norm(dim=-1) * k[:, h].norm(dim=-1)).min()) > 160
    a64 = L.cached(c)[5]
    v_mean = torch.stack([(fuser.query.double() @ ml.self_attn.in_proj_weight.double()[32:].T
                           + ml.self_attn.in_proj_bias.double()[32:]).mean(0)
                          for ml in fuser.mpfusion["fusion0"].ml_fusion_layers.values()])
    torch.testing.assert_close(a64[:, :, 2 * h:2 * h + 2], v_mean[:, None, 2 * h:2 * h + 2].expand(-1, c.Q, -1), rtol=1e-12, atol=1e-12)
    # scores-split: a slice is redone for the queries on the other side of the split, and only for them; the slice that holds
    # the split is ordinary for everyone; the pair that straddles the split has one query of each kind
    c = L.by_name("scores-split")
    fuser = L.cached(c)[0]
    q, k = L.qk_rows(fuser, 0)
    den = L.slice_log2_den(q, k, NS)[0, h]                     # (Q,NS)
    SL = math.ceil(c.Q / NS)
    qside = torch.arange(c.Q) < L.SPLIT_AT
    n_fb = 0
    for sl in range(NS):
        k0, k1 = sl * SL, min(c.Q, (sl + 1) * SL)
        assert k1 > k0
        kside = {bool(x) for x in (torch.arange(k0, k1) < L.SPLIT_AT)}
        for qi in range(c.Q):
            if len(kside) == 2 or bool(qside[qi]) in kside:
                assert float(den[qi, sl]) > -50, (qi, sl, float(den[qi, sl]))
            else:
                assert float(den[qi, sl]) < -300, (qi, sl, float(den[qi, sl]))
                n_fb += 1
    assert n_fb > c.Q * (NS - 1) * 0.4
    pair = L.SPLIT_AT - 1
    assert pair % 2 == 0 and bool(qside[pair]) != bool(qside[pair + 1])
    assert float(L.slice_log2_den(q, k, NS)[0, [m for m in range(8) if m != h]].min()) > -50


def test_supported_follows_the_librarys_limit():
    from dpft_amd.models.fusers import fused
    QC, NS, XR, QMAX = L.limits()
    assert fused.limits() == (QC, NS, XR, QMAX)
    for c in L.CASES:
        assert fused.supported(L.cached(c)[0]), c.name
    big = L.make_fuser(L.by_name("q1")._replace(name="over", Q=QMAX + 1))
    assert not fused.supported(big)
    edge = L.make_fuser(L.by_name("q1")._replace(name="edge", Q=QMAX))
    assert fused.supported(edge)
