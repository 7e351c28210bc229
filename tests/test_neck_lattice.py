"""The lattice of the FPN neck (tests/neck_lattice.py), checked without a GPU: the case table reaches what it claims, the float
index rule restated in numpy is F.interpolate's and differs from the exact rule at the pairs the table names, the backward
kernel's candidate window contains every destination of its source pixel for all size pairs below 700, the fp32 yardstick is
finite and small, and the table of exactly-zero gradients is what torch's autograd of the oracle gives.  The GPU half is
tests/test_gpu_neck_lattice.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dprt_oracle as O
from tests import neck_lattice as L


def test_table_reaches_what_it_claims():
    c = {x.name: x for x in L.CASES}
    assert len(c) == len(L.CASES) == 7
    for x in L.CASES:
        assert x.B <= 3 and len(x.in_ch) == len(x.sizes) and x.out % 4 == 0, x.name
        assert all(H >= TH and W >= TW for _, H, TH, W, TW in L.pairs(x)), x.name      # the kernels' TH <= H, TW <= W
        assert len(L.param_names(x)) == 4 * L.n_levels(x)
    # every predicate holds for at least one case, and for the case the table names
    for p in L.PREDICATES:
        assert any(p(x) for x in L.CASES), p.__name__
    assert L.float_rule_on_fused_lateral(c["radar-5"]) and L.fused_c6(c["radar-5"]) and L.top_is_one_pixel(c["radar-5"])
    assert L.g_prev_chain(c["radar-5"]) == 5 and max(L.g_prev_chain(x) for x in L.CASES) == 5
    assert L.fused_c3(c["camera-3"]) and L.thin_wgrad_with_bias(c["camera-3"], 0) and L.ragged_conv16_tiles(c["camera-3"])
    assert L.g_prev_chain(c["camera-3"]) == 3
    assert L.float_rule_on_generic_lateral(c["float-rule-generic"]) and not L.fused_lateral(c["float-rule-generic"], 0)
    assert not L.float_rule_on_generic_lateral(c["radar-5"]) and not L.float_rule_on_fused_lateral(c["float-rule-generic"])
    assert L.same_size_both(c["same-size"]) and L.same_height_only(c["same-size"])
    assert L.fused_lateral(c["same-size"], 0) and not L.fused_lateral(c["same-size"], 1)      # one of each kernel
    assert L.one_level(c["single"]) and list(L.cot_sets(c["single"])) == ["all"]
    for name in ("k32", "k8"):          # no thin path: neither lateral, nor embedding, nor weight gradient
        x = c[name]
        assert not L.fused_embedding(x) and not any(L.fused_lateral(x, i) or L.thin_wgrad_with_bias(x, i) for i in range(L.n_levels(x)))
    assert L.wide_neck(c["k32"]) and L.narrow_neck(c["k8"]) and c["k8"].out == 8 and L.embedding_kwargs(c["k8"])["num_feats"] == 8
    assert set(L.FLOAT_RULE) == {x.name for x in L.CASES if L.float_rule_on_fused_lateral(x) or L.float_rule_on_generic_lateral(x)}
    assert set(L.CHILD) == {"radar-5", "camera-3"}
    # cotangent sets: the top only, level 0 only, all but the middle level
    assert L.cot_sets(c["radar-5"]) == dict(all=(0, 1, 2, 3, 4), top=(4,), level0=(0,), **{"no-mid": (0, 1, 3, 4)})
    assert L.cot_sets(c["camera-3"])["no-mid"] == (0, 2)
    # the kernel-level case takes a second step of the grid-stride loop; every module case stays within the first
    k = L.KERNEL_CASE
    assert L.TO16_CAP < k["B"] * k["H"] * k["W"] < 2 * L.TO16_CAP and (k["C"], k["K"]) == (3, 16)
    assert all(x.B * h * w < L.TO16_CAP for x in L.CASES for h, w in x.sizes)


def test_float_rule_cases_contain_a_destination_the_exact_rule_maps_elsewhere():
    want = {"radar-5": {(46, 14): [23], (44, 26): [22]}, "float-rule-generic": {(58, 30): [29], (46, 28): [23]}}
    for name in L.FLOAT_RULE:
        c = L.by_name(name)
        found = {}
        for _, H, TH, W, TW in L.pairs(c):
            for n_out, n_in in ((H, TH), (W, TW)):
                d = L.rule_differs(n_out, n_in)
                if d:
                    found[(n_out, n_in)] = d
        assert found == want[name], (name, found)
    assert (L.float_src(46, 14)[23], L.exact_src(46, 14)[23]) == (6, 7)
    assert (L.float_src(44, 26)[22], L.exact_src(44, 26)[22]) == (12, 13)
    # the smallest pairs at which the two rules part; no other case of the table has one
    assert [(o, i) for o in range(2, 59) for i in range(1, o) if L.rule_differs(o, i)] == [(44, 26), (46, 14), (46, 28), (58, 30)]
    for c in L.CASES:
        if c.name not in L.FLOAT_RULE:
            assert not any(L.rule_differs(H, TH) or L.rule_differs(W, TW) for _, H, TH, W, TW in L.pairs(c)), c.name


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_numpy_rule_is_interpolates(dtype):
    """F.interpolate(mode="nearest") follows the float rule for fp32 and for fp64 inputs (so the fp64 oracle is the reference at
    the float-rule pairs), and oracle.nearest_index is the same rule."""
    sizes = [(46, 14), (44, 26), (58, 30), (46, 28), (40, 20), (57, 29), (37, 10), (3, 1), (9, 9)]
    sizes += [(k["H"], k["TH"]) for k in [L.KERNEL_CASE]] + [(L.KERNEL_CASE["W"], L.KERNEL_CASE["TW"])]
    for n_out, n_in in sizes:
        src = torch.arange(n_in, dtype=dtype).view(1, 1, n_in, 1)
        got = F.interpolate(src, size=(n_out, 1), mode="nearest").flatten().long().numpy()
        assert np.array_equal(got, L.float_src(n_out, n_in)), (n_out, n_in)
        got = F.interpolate(src.view(1, 1, 1, n_in), size=(1, n_out), mode="nearest").flatten().long().numpy()
        assert np.array_equal(got, L.float_src(n_out, n_in)), (n_out, n_in)
    for n_out, n_in in sizes[:4]:
        assert [O.nearest_index(d, n_in, n_out) for d in range(n_out)] == L.float_src(n_out, n_in).tolist()


def test_backward_candidate_window_contains_every_destination():
    """fpn_topdown_add_bwd_kernel searches floorf(th / sh) - 2 .. ceilf((th + 1) / sh) + 2 for the destinations of source th and
    filters them by the forward rule: the window has to contain them all, or a gradient is dropped.  All 1 <= in < out < 700."""
    for n_out in range(2, 700):
        assert L.window_misses(n_out) == [], n_out
    # the all-sizes form above is the per-pair one
    for n_out, n_in in ((46, 14), (44, 26), (699, 1), (699, 698), (100, 33), (520, 260)):
        lo, hi = L.candidate_window(n_out, n_in)
        src, dst = L.float_src(n_out, n_in), np.arange(n_out)
        assert bool(((dst >= lo[src]) & (dst <= hi[src])).all()), (n_out, n_in)
        assert set(src.tolist()) == set(range(n_in))            # every source has a destination: none is skipped going up
    # and it is a window, not the whole axis
    lo, hi = L.candidate_window(699, 350)
    assert int((hi - lo).max()) <= 8


@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_yardstick_is_finite_and_zero_gradients_are_the_tables(c):
    sd, xs, cots, e64, e32 = L.cached(c)
    print(L.report(c))
    assert sorted(sd) == sorted(L.param_names(c))
    assert all(float(v.abs().min()) > 0 for k, v in sd.items() if k.endswith("bias")), "non-zero biases"
    assert [tuple(x.shape) for x in xs] == L.level_shapes(c) and [tuple(t.shape) for t in cots] == L.out_shapes(c)
    assert [tuple(v.shape) for v in e64["outs"]] == L.out_shapes(c)
    for a, b in zip(e32["outs"] + e32["neck"], e64["outs"] + e64["neck"]):
        assert a.dtype == torch.float32 and b.dtype == torch.float64 and bool(torch.isfinite(a).all())
        assert L.rel_l2(a, b) < 2e-6 and L.rel_max(a, b) < 2e-6          # the case does not amplify round-off
    assert list(e64["grads"]) == list(L.cot_sets(c))
    names = L.param_names(c) + [f"x{i}" for i in range(L.n_levels(c))]
    for key, levels in L.cot_sets(c).items():
        g64, g32 = e64["grads"][key], e32["grads"][key]
        assert sorted(g64) == sorted(names)
        zero = {k for k, g in g64.items() if not bool(g.any())}
        assert zero == L.zero_grads(c, levels) == {k for k, g in g32.items() if not bool(g.any())}, (c.name, key, zero)
        for k, g in g64.items():
            assert bool(torch.isfinite(g32[k]).all()), (c.name, key, k)
            if k not in zero:
                assert L.rel_l2(g32[k], g) < 5e-6 and L.rel_max(g32[k], g) < 5e-6, (c.name, key, k)
    assert L.zero_grads(c, L.cot_sets(c)["all"]) == set()


def test_oracle_reads_the_float_rule_source_at_the_named_destinations():
    """The upsample the fp64 oracle calls distinguishes the two rules on radar-5's own sizes: destination row 23 of level 0 reads
    source row 6 of level 1 (exact rule: 7), destination column 22 reads source column 12 (exact rule: 13)."""
    c = L.by_name("radar-5")
    lat1 = torch.randn(c.B, c.out, *c.sizes[1], dtype=torch.float64, generator=torch.Generator().manual_seed(0)).requires_grad_(True)
    up = F.interpolate(lat1, size=c.sizes[0], mode="nearest")
    g, = torch.autograd.grad(up[:, :, 23, :].sum(), lat1, retain_graph=True)
    assert g.abs().sum((0, 1, 3)).nonzero().flatten().tolist() == [6]
    g, = torch.autograd.grad(up[:, :, :, 22].sum(), lat1)
    assert g.abs().sum((0, 1, 2)).nonzero().flatten().tolist() == [12]
