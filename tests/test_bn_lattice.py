"""The BatchNorm pass lattice (tests/bn_lattice.py) checked without a GPU: it covers the dispatch classes it claims, its fp64
reference equals the definition written as plain loops, its exact tier is exact in float32 for every kernel expression, the float
tier's bound holds for a float32 replay (the new C entries' refusals: tests/test_host.py).  The GPU half is
tests/test_gpu_bn_passes.py."""
import collections

import pytest
import torch

from tests import bn_lattice as L


def test_lattice_is_deterministic_and_no_dispatch_class_is_empty():
    assert L.build_lattice() == L.LATTICE and L.build_pool_lattice() == L.POOL_LATTICE
    assert {c.K for c in L.LATTICE} >= set(L.K_VALUES)
    count = collections.Counter(t for c in L.LATTICE for t in L.case_tags(c))
    print("lattice: %d cases; per class: %s" % (len(L.LATTICE), dict(sorted(count.items()))))
    assert not (L.REQUIRED_TAGS - set(count)), sorted(L.REQUIRED_TAGS - set(count))
    for changed in L.SWITCH_RUNS:
        key = ",".join("%s=%d" % kv for kv in changed.items())
        got = {t for c in L.LATTICE for t in L.case_tags(c, L.switches(**changed))}
        want = L.REQUIRED_TAGS_BY_SWITCH.get(key, set())
        assert not (want - got), (key, sorted(want - got))
    assert max(c.M * c.K for c in L.LATTICE) * 4 <= 9 << 20                       # the largest tensor: a few MB
    # pool: both backward kernels, one tile +- 1 in both directions, 1 to 3 pixels
    forms = collections.Counter(L.pool_bwd_form(c.H, c.W, c.K, L.DEFAULT_SWITCHES) for c in L.POOL_LATTICE)
    assert forms["pool_tiled"] >= 8 and forms["generic"] >= 8
    assert {c.H for c in L.POOL_LATTICE} >= {1, 2, 3, 2 * L.PB_TH - 1, 2 * L.PB_TH, 2 * L.PB_TH + 1}
    assert {c.W for c in L.POOL_LATTICE} >= {1, 2, 3, 2 * L.PB_TW - 1, 2 * L.PB_TW, 2 * L.PB_TW + 1}
    sums = collections.Counter((L.sums_launch(c.M, c.K, L.DEFAULT_SWITCHES), c.K // 4 < 256) for c in L.SUMS_CASES)
    assert sums[("sums_taken", True)] >= 2 and sums[("sums_taken", False)] >= 2 and sums[("sums_declined", True)] >= 2


def test_reference_equals_plain_loops_on_tiny_cases():
    for c in (L.Case("tiny-a", 3, 4), L.Case("tiny-b", 2, 8), L.Case("tiny-c", 5, 12)):
        o = L.exact_operands(c)
        y, res, d, b, rb, ga = (o[k].tolist() for k in ("y", "res", "dout", "bnp", "rbnp", "gamma"))
        out = L.ref_act(o["y"], o["bnp"], o["res"], o["rbnp"], True)
        m8 = L.mask_bytes(out)
        sums = L.ref_reduce(o["y"], o["dout"], o["bnp"], out > 0)
        dy = L.ref_apply(o["y"], o["dout"], o["bnp"], o["gamma"], sums, out > 0, False)
        dyf = L.ref_apply(o["y"], o["dout"], o["bnp"], o["gamma"], sums, out > 0, True)
        s0, s1 = [0.0] * c.K, [0.0] * c.K
        for m in range(c.M):
            for k in range(c.K):
                v = max((y[m][k] - b[0][k]) * b[1][k] + b[2][k] + (res[m][k] - rb[0][k]) * rb[1][k] + rb[2][k], 0.0)
                assert out[m, k].item() == v and ((int(m8[m, k // 4]) >> (k % 4)) & 1) == (v > 0)
                dz = d[m][k] if v > 0 else 0.0
                s0[k] += dz
                s1[k] += dz * (y[m][k] - b[0][k]) * b[3][k]
        assert sums.tolist() == [s0, s1]
        for m in range(c.M):
            for k in range(c.K):
                dz = d[m][k] if out[m, k] > 0 else 0.0
                xh = (y[m][k] - b[0][k]) * b[3][k]
                assert dy[m, k].item() == pytest.approx(ga[k] * b[3][k] * (dz - s0[k] / c.M - xh * s1[k] / c.M), abs=1e-12)
                assert dyf[m, k].item() == ga[k] * b[3][k] * dz
    # pool: one hand-made map; the tie goes to the FIRST maximum in window scan order, nothing to a window whose maximum is 0
    y = torch.tensor([[2.0, 2.0, -1.0], [2.0, -1.0, -1.0], [-1.0, -1.0, -1.0]]).double().reshape(1, 3, 3, 1).repeat(1, 1, 1, 4)
    bnp = torch.tensor([[0.0] * 4, [1.0] * 4, [0.0] * 4, [1.0] * 4]).double()
    out, arg = L.ref_pool(y, bnp)
    assert out[0, :, :, 0].tolist() == [[2.0, 2.0], [2.0, 0.0]]
    dout = torch.tensor([[1.0, 10.0], [100.0, 1000.0]]).double().reshape(1, 2, 2, 1).repeat(1, 1, 1, 4)
    dz = L.ref_pool_bwd(y, bnp, dout)
    assert dz[0, :, :, 0].tolist() == [[1.0, 10.0, 0.0], [100.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    assert not torch.equal(L.ref_pool(y, bnp, last_max=True)[1], arg)              # the other tie rule is a different answer
    s = L.encode_sums(torch.tensor([-7.0, 9.5], dtype=torch.float64), torch.tensor([0.25, 2.0 ** 40 + 3], dtype=torch.float64))
    back = s[0::2].double() * 4.0 + s[1::2].double() * 2.0 ** -46
    assert back.tolist() == [[-7.0, 9.5], [0.25, 2.0 ** 40 + 3]]


def test_exact_tier_is_exact_in_float32_for_every_kernel_expression():
    # nothing is ever dropped or rescaled: the operand ranges make every case exact, and a case that were not fails here
    for c in L.LATTICE + list(L.SUMS_CASES):
        L.exact_proof(c)
    # the train-mode apply carries real sums wherever 1 / M is exact, in every elementwise dispatch class
    with_sums = {(L.elementwise_launch("apply", c.M, c.K, b, L.DEFAULT_SWITCHES).form, b)
                 for c in L.LATTICE if L.apply_sums_exact(c.M) for b in (False, True)}
    assert with_sums >= {("generic", False), ("fixc2", False), ("generic", True), ("wide16", True), ("wide16_fixc", True)}
    for c in L.POOL_LATTICE:
        o = L.pool_operands(c)
        out, arg = L.ref_pool(o["y"], o["bnp"])
        assert bool((out.bfloat16().double() == out).all()) and bool((L.ref_pool_bwd(o["y"], o["bnp"], o["dout"]).abs() <= 12).all())
    ties = sum(int((L.ref_pool(o["y"], o["bnp"])[1] != L.ref_pool(o["y"], o["bnp"], last_max=True)[1]).sum())
               for o in map(L.pool_operands, L.POOL_LATTICE))
    assert ties > 1000                                     # windows where first and last maximum differ


def test_float_tier_bound_holds_for_the_float32_replay():
    """Both kernel expressions stay within the bound with c halved; the uncentred fixed-channel form the kernels used before
    (FOUND AND FIXED in tests/bn_lattice.py) does not."""
    for c in L.FLOAT_CASES:
        w = L.float_selfcheck(c)
        print(c.name, {k: float("%.3g" % v) for k, v in w.items()})
        for k, v in w.items():
            if not k.startswith("fixc-uncentred") or ":frozen" in k:
                assert v <= (2.0 if c.name in L.SELFCHECK_FULL_BOUND_ONLY else 1.0), (c.name, k, v)      # (ratios are to c / 2)
        assert w["fixc-uncentred:r1000"] > 100 * w["fixc:r1000"], (c.name, w)
