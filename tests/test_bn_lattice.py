"""The BatchNorm pass lattice (tests/bn_lattice.py) checked without a GPU: it covers the dispatch classes it claims, its fp64
reference equals the definition written as plain loops, its exact tier is exact in float32 for every kernel expression, the float
tier's bound holds for a float32 replay (the new C entries' refusals: tests/test_host.py), and the library's launch plans
(dpft_bn_plan_query, host only) equal the restated dispatch under every switch set.  The GPU half is tests/test_gpu_bn_passes.py."""
import collections
import ctypes as C
import os

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


PASS_ACT, PASS_ACT_SUMS, PASS_REDUCE, PASS_APPLY, PASS_POOL_BWD = range(5)      # DPFT_BN_PASS_*
PLAN_OUT32, PLAN_ALIGNED16 = 1, 2                                               # DPFT_BN_PLAN_*


def _plan(lib, pas, M, K, sw, bf16=False, flags=0, H=0, W=0):
    from dpft_amd.hip.lib import BnPlan, BnSwitches
    switches = BnSwitches(sw["fixc"], sw["wide16"], sw["fat"], sw["tiled"], sw["per_cu"])
    plan = BnPlan()
    lib.call("dpft_bn_plan_query", pas, M, K, H, W, int(bf16), flags, C.byref(switches), C.byref(plan))
    return plan


def test_planned_launch_is_the_restated_dispatch_under_every_switch_set():
    """The plan every BatchNorm pass launches from (bn_plan.h, asked through dpft_bn_plan_query: nothing is launched) against the
    restatement of tests/bn_lattice.py: form, block count (with it the trim) and quads per thread of act and apply, taken /
    declined, grid and LDS bytes of the column-sums pass, the reduce geometry, the pool backward's form -- for every case, both
    storage types, with and without the fp32 copy, under the default switches and each one-switch change.  Integers: all exact."""
    from dpft_amd.hip.lib import BnPlan, lib
    from dpft_amd.hip.ops import BN_FORMS
    cases = L.LATTICE + list(L.SUMS_CASES)
    hit, compared = collections.Counter(), 0
    for sw in [L.switches()] + [L.switches(**changed) for changed in L.SWITCH_RUNS]:
        for c in cases:
            for kind, pas in (("act", PASS_ACT), ("apply", PASS_APPLY)):
                for bf16 in (False, True):
                    for out32 in (False, True):
                        want = L.elementwise_launch(kind, c.M, c.K, bf16, sw, out32)
                        got = _plan(lib, pas, c.M, c.K, sw, bf16, PLAN_ALIGNED16 | (PLAN_OUT32 if out32 else 0))
                        assert (BN_FORMS[got.form], got.grid_x, got.grid_y, got.per_thread, got.lds_bytes) == \
                               (want.form, want.blocks, 1, want.per_thread, 0), (c, kind, bf16, out32, sw)
                        hit[(kind, want.form)] += 1
                        compared += 1
                # tensors off 16 bytes: bf16 storage falls back to the 8-byte kernel, whatever the switches
                want = L.elementwise_launch(kind, c.M, c.K, True, dict(sw, wide16=0))
                got = _plan(lib, pas, c.M, c.K, sw, True, 0)
                assert want.form == "generic" and (BN_FORMS[got.form], got.grid_x, got.per_thread) == ("generic", want.blocks, 2), (c, kind, sw)
            form = L.sums_launch(c.M, c.K, sw)
            got = _plan(lib, PASS_ACT_SUMS, c.M, c.K, sw)
            assert BN_FORMS[got.form] == form, (c, sw)
            if form == "sums_taken":
                assert (got.grid_x, got.per_thread, got.lds_bytes) == (L.f32_fixc(c.M, c.K, sw)[1], min(sw["fixc"], 2), L.sums_lds_bytes(c.K)), (c, sw)
            else:
                assert (got.grid_x, got.lds_bytes) == (0, 0), (c, sw)                     # nothing is launched
            hit[("sums", form[5:])] += 1
            for bf16 in (False, True):
                g = L.reduce_geometry(c.M, c.K, bf16)
                got = _plan(lib, PASS_REDUCE, c.M, c.K, sw, bf16)
                assert (BN_FORMS[got.form], got.slab, got.slabs, got.groups, got.rows_per_block, got.grid_x, got.grid_y, got.per_thread) == \
                       ("generic", g["slab"], g["slabs"], g["groups"], g["rows_per_block"], g["grid_x"], g["slabs"], g["RT"]), (c, bf16)
        for c in L.POOL_LATTICE:
            for bf16 in (False, True):
                got = _plan(lib, PASS_POOL_BWD, c.B, c.K, sw, bf16, H=c.H, W=c.W)
                assert BN_FORMS[got.form] == L.pool_bwd_form(c.H, c.W, c.K, sw), (c, sw)
    print("element-wise comparisons: %d; per (pass, form): %s" % (compared, dict(sorted(hit.items()))))
    assert compared == len(cases) * 8 * 8
    want_classes = {("act", f) for f in ("fixc1", "fixc2", "generic", "wide16", "wide16_fixc")} | \
                   {("apply", f) for f in ("fixc1", "fixc2", "fixc3", "generic", "wide16", "wide16_fixc")} | \
                   {("sums", "taken"), ("sums", "declined")}
    assert set(hit) == want_classes, sorted(set(hit) ^ want_classes)
    # NULL switches: the process's own (the defaults, unless the environment of this run changes them)
    c, plan = L.by_name("sums-k1024"), BnPlan()
    lib.call("dpft_bn_plan_query", PASS_APPLY, c.M, c.K, 0, 0, 0, 0, None, C.byref(plan))
    want = L.elementwise_launch("apply", c.M, c.K, False, L.switches_from_env(os.environ))
    assert (BN_FORMS[plan.form], plan.grid_x, plan.per_thread) == (want.form, want.blocks, want.per_thread)
    # refusals: nothing is written through a bad call
    assert lib.dpft_bn_plan_query(PASS_ACT, 16, 64, 0, 0, 0, 0, None, None) == -1 and b"plan is null" in lib.dpft_last_error()
    assert lib.dpft_bn_plan_query(5, 16, 64, 0, 0, 0, 0, None, C.byref(plan)) == -1 and b"unknown pass" in lib.dpft_last_error()
    assert lib.dpft_bn_plan_query(PASS_ACT, 16, 66, 0, 0, 0, 0, None, C.byref(plan)) == -1 and b"bad shape" in lib.dpft_last_error()
    assert lib.dpft_bn_plan_query(PASS_ACT, 16, 64, 0, 0, 2, 0, None, C.byref(plan)) == -1 and b"storage" in lib.dpft_last_error()
    assert lib.dpft_bn_plan_query(PASS_ACT_SUMS, 16, 64, 0, 0, 1, 0, None, C.byref(plan)) == -1 and b"fp32 only" in lib.dpft_last_error()
    assert lib.dpft_bn_plan_query(PASS_POOL_BWD, 2, 64, 0, 8, 0, 0, None, C.byref(plan)) == -1 and b"bad pool shape" in lib.dpft_last_error()
