"""The lattice of the ResNet launch plan (tests/plan_lattice.py), checked without a GPU: the case table reaches the plan decisions
it claims, the one fp64 walk equals oracle.dprt_oracle.resnet_body when no hook is set, and every (case, BatchNorm mode) is
conditioned so that the GPU half can hold the plan to fp32 round-off: no ReLU input and no max-pool decision within 8x the fp32
oracle's own deviation of a flip, and the fp32 oracle within 2e-5 (outputs) / 2e-4 (every parameter gradient) of its fp64 value,
so that no case is ill-conditioned enough to hide a kernel error behind the 4 e32 of the bound.  These are conditions of the
inputs, asserted; the measured margins are printed.  The GPU half is tests/test_gpu_plan_lattice.py."""
import pytest
import torch
import torch.nn.functional as F

from oracle import dprt_oracle as O
from tests import plan_lattice as L


def test_table_reaches_what_it_claims():
    c = {x.name: x for x in L.CASES}
    assert len(c) == len(L.CASES)
    for x in L.CASES:
        assert len(x.depths) == x.multi_scale <= 4 and all(1 <= n <= 3 for n in x.depths), x.name
        # every BatchNorm sees at least 4 rows: at M = 3 the fp32 oracle alone is off by 1e-1 in the gradients
        assert all(m >= 4 for _, _, m, _ in L.bn_layers(x)), (x.name, L.bn_layers(x))
        assert len(L.bn_layers(x)) == 1 + sum(3 * n + 1 for n in x.depths)
        assert L.n_convs(x) == len(L.bn_layers(x)) + (x.in_ch != 3)
    geo = {x.name: L.geometry(x) for x in L.CASES}
    # odd and even stem and pool sizes
    stem_sizes = {n % 2 for g in geo.values() for n in g[0]}
    pool_sizes = {n % 2 for g in geo.values() for n in g[1]}
    assert stem_sizes == {0, 1} and pool_sizes == {0, 1}
    assert geo["odd-wide"][:2] == ((17, 35), (9, 18)) and geo["l4-2x1"][:2] == ((18, 14), (9, 7))
    assert geo["odd-wide"][2] == [(9, 18), (5, 9), (3, 5), (2, 3)]
    assert all(n % 2 == 0 for hw in (geo["even-2x2"][0], geo["even-2x2"][1], *geo["even-2x2"][2]) for n in hw)
    # a 1x1 layer4 map (once behind a second block), a 2x1 one with the smallest admitted M, a batch of one
    assert geo["b4-1x1"][2][3] == (1, 1) and geo["parity"][2][3] == (1, 1) and c["parity"].depths[3] == 2
    assert geo["l4-2x1"][2][3] == (2, 1) and min(m for _, _, m, _ in L.bn_layers(c["l4-2x1"])) == 4
    assert c["b1"].B == 1
    assert {x.multi_scale for x in L.CASES} == {1, 2, 3, 4} and {x.in_ch for x in L.CASES} == {3, 6}
    # a stage of three blocks: the bn3 reduction of the next block is folded twice, two residual data gradients without a downsample
    assert 3 in c["l1only"].depths and c["l1only"].multi_scale == 1
    # both parities of "blocks in later stages" for every stage index that has later stages; the last stage always starts at 0
    parities = {li: set() for li in range(4)}
    for x in L.CASES:
        for li, n in enumerate(L.later_blocks(x)):
            parities[li].add(n & 1)
        assert L.later_blocks(x)[-1] == 0
    assert parities[0] == parities[1] == parities[2] == {0, 1} and parities[3] == {0}, parities
    assert [L.later_blocks(c[n]) for n in ("odd-wide", "parity")] == [[4, 3, 1, 0], [5, 3, 2, 0]]
    # statistics rows: below one tile, several tiles with a ragged last one, exact multiples
    rows = {m for x in L.CASES for _, _, m, _ in L.bn_layers(x)}
    assert min(rows) == 4 and max(rows) == 2048 and {128, 512, 2048} <= rows and {324, 1190} <= rows
    # the partial-cotangent and bf16 subsets: multi_scale 4, 3 and 1 and both parity patterns; even, odd and single-stage
    assert {c[n].multi_scale for n in L.PARTIAL} == {1, 3, 4} and {"odd-wide", "parity"} <= set(L.PARTIAL)
    assert set(L.BF16) == {"even-2x2", "odd-wide", "l1only"}
    for n in L.PARTIAL:
        sets = L.cot_sets(c[n])
        assert sets["last"] == (len(c[n].depths) - 1,) and (len(c[n].depths) == 1 or sets["mid"] == (1,))


def test_widest_gap_rule():
    """beta lands in the middle of the widest gap among the nearest zeros, also beyond the outermost one."""
    v = -torch.tensor([[0.0, 1.0, 1.5, 4.0, 4.1, 4.2, 9.0], [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0]], dtype=torch.float64)
    got = L._widest_gap_beta(v, torch.tensor([1.4, -7.0], dtype=torch.float64))
    assert float(got[0]) == 2.75                    # zeros 0, 1, 1.5 | 4, 4.1, 4.2 around 1.4: the gap 1.5 .. 4
    assert float(got[1]) == -0.5                    # below every zero: one mean gap (1) under the lowest
    one = L._widest_gap_beta(-torch.tensor([[2.0]], dtype=torch.float64), torch.tensor([2.0], dtype=torch.float64))
    assert abs(float(one[0]) - 2.0) > 1e-4


def test_quantiser_is_exact_on_bf16_operands():
    """On operands and cotangents that are bf16 values already, the quantised conv is F.conv2d, output and both gradients."""
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(torch.bfloat16).double()
    x, w, cot = r(2, 64, 5, 4), r(8, 64, 3, 3), r(2, 8, 3, 2)
    got, ref = [], []
    for fn, out in ((lambda a, b: L.quant_conv(a, b, "c", stride=2, padding=1), got), (lambda a, b: F.conv2d(a, b, stride=2, padding=1), ref)):
        a, b = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        y = fn(a, b)
        out += [y.detach(), *torch.autograd.grad((y * cot).sum(), [a, b])]
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    # and it rounds: operands off the bf16 grid change the result; a conv with C % 64 != 0 is left alone
    x2 = x + 1e-4
    assert not torch.equal(F.conv2d(x2, w, stride=2, padding=1), L.quant_conv(x2, w, "c", stride=2, padding=1))
    assert torch.equal(F.conv2d(x2[:, :3], w[:, :3]), L.quant_conv(x2[:, :3], w[:, :3], "c"))
    t = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], dtype=torch.float64)      # ties: to even
    assert L._round_bf16(t).tolist() == [1.0, 1.0 + 2.0 ** -6]


def test_running_statistics_rule_is_batch_norms():
    """running_stats() against what torch.nn.functional.batch_norm leaves in its buffers after one and two calls."""
    c = L.by_name("l1only")
    sd, x, e64, _ = L.cached(c, "train")
    for name in ("body.bn1", "body.layer1.2.bn3"):
        y = e64["taps"]["bn_in"][name]
        rm, rv = sd[f"{L.P}.{name}.running_mean"].double().clone(), sd[f"{L.P}.{name}.running_var"].double().clone()
        for steps in (1, 2):
            F.batch_norm(y, rm, rv, None, None, training=True, momentum=L.MOMENTUM, eps=L.EPS)
            ref = L.running_stats(c, sd, {name: y}, steps)[name]
            torch.testing.assert_close(ref[0], rm, rtol=1e-13, atol=1e-13)
            torch.testing.assert_close(ref[1], rv, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_hook_free_walk_is_the_oracle_body(c):
    sd32, x = L.cached(c, "train")[:2]
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd32.items()}
    xin = L._body_input(x.double(), sd)
    for train in (True, False):
        ref = O.resnet_body(xin, sd, L.P + ".body", c.depths, train, c.multi_scale)
        got = L.walk(xin, sd, L.P + ".body", c.depths, train, c.multi_scale)
        assert list(got) == list(ref) == [str(i + 1) for i in range(c.multi_scale)]
        assert all(torch.equal(got[k], ref[k]) for k in ref), c.name
    # and the evaluation built on it is oracle.backbone's layout: NHWC stage outputs of the lattice's shapes
    outs = L.cached(c, "train")[2]["outs"]
    assert [tuple(v.shape) for v in outs.values()] == L.stage_shapes(c)


@pytest.mark.parametrize("mode", L.MODES)
@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_case_is_well_conditioned(c, mode):
    sd, x, e64, e32 = L.cached(c, mode)
    print(L.report(c, mode))
    # every tensor is an fp32 value; the conditioning moved the biases of the BatchNorms that feed a ReLU and nothing else
    drawn = L.drawn_state(c)[0]
    relu_bias = {f"{L.P}.{n}.bias" for n, _, _, relu in L.bn_layers(c) if relu}
    for k, v in sd.items():
        assert v.dtype in (torch.float32, torch.int64), k
        assert torch.equal(v, drawn[k]) != (k in relu_bias), k
    assert x.dtype == torch.float32 and float(x.max()) > 200
    # ReLU inputs: min |x| in fp64 at least 8x the fp32 oracle's deviation at that tensor, equal sign patterns
    rows = L.relu_margins(e64["taps"]["relu_in"], e32["taps"]["relu_in"])
    assert len(rows) == sum(relu for _, _, _, relu in L.bn_layers(c))
    for name, lo, dev, same in rows:
        assert same and lo >= L.MARGIN * dev, (c.name, mode, name, lo, dev)
    # the stem max-pool: no window with a positive maximum whose two largest entries are closer than 8x the deviation
    gap, dev = L.pool_margin(e64["taps"]["pool_in"]["body.bn1"], e32["taps"]["pool_in"]["body.bn1"])
    assert gap >= L.MARGIN * dev, (c.name, mode, gap, dev)
    # the case does not amplify round-off: caps on the fp32 oracle's own error
    for k, v in e64["outs"].items():
        assert L.rel_l2(e32["outs"][k], v) <= L.CAP_OUT, (c.name, mode, k, L.rel_l2(e32["outs"][k], v))
    for s, grads in e64["grads"].items():
        later = [k for k, g in grads.items() if float(g.norm()) == 0]
        assert (s == "mid" and len(c.depths) > 2) == bool(later), (c.name, s, later)      # zero only behind the last cotangent
        assert all(k.startswith("body.layer") and int(k.split(".")[1][5:]) - 1 > max(L.cot_sets(c)[s]) for k in later)
        for k, g in grads.items():
            if k not in later:
                assert L.rel_l2(e32["grads"][s][k], g) <= L.CAP_GRAD, (c.name, mode, s, k, L.rel_l2(e32["grads"][s][k], g))
