"""Deep supervision, kernels and ``Loss``: the layered matcher cost, assignment, criterion and gradient entries
(dpft_*_layers_f32, dpft_amd/csrc/misc.hip) against the single-output entries they generalise -- bit for bit, layer by layer --
and against the fp64 restatement of tests/aux_loss_ref.py; then ``Loss`` with ``aux_weights`` on synthetic outputs.

Every layer of a case lives in its own allocation, as the decoder graph's static buffers do."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import aux_loss_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
KEYS = ("class", "center", "size", "angle")
COST_W = (1.0, 1.0, 2.0, 1.0, 1.0)                         # total_class, center, size, angle, GIoU
W = {"total_class": 1.0, "object_class": 0.5, "center": 1.0, "size": 2.0, "angle": 1.0}
W5 = tuple(W[k] for k in R.TERMS)
ALPHA = 0.75
CYCLE = (1.0, 0.5, 0.3)

# (L, B, N, Mmax, C, counts)
LATTICE = [
    (1, 1, 5, 3, 1, (3,)),
    (2, 2, 12, 4, 3, (4, 0)),
    (3, 2, 3, 5, 2, (5, 2)),                               # more targets than queries
    (4, 3, 100, 7, 2, (7, 1, 0)),                          # B * N = 300: a full block plus a tail in every layer
    (8, 2, 400, 9, 8, (9, 3)),                             # four blocks per layer, the table full
]
SMALL = LATTICE[:3]
IDS = ["L%d-B%d-N%d-M%d-C%d" % c[:5] for c in LATTICE]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def close(a, b, rtol=1e-4, atol_scale=1e-5, what=""):
    """The rule of tests/test_gpu_model.py::test_loss_and_matcher_match_oracle."""
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    atol = atol_scale * max(float(b.abs().max()), 1e-6)
    torch.testing.assert_close(a, b, rtol=rtol, atol=atol, msg=lambda m: f"{what}: {m}")


def _make(spec):
    L, B, N, Mmax, ncls, counts = spec
    g = torch.Generator().manual_seed(100 * L + N)
    layers = []
    for _ in range(L):
        layers.append({"center": torch.randn(B, N, 3, generator=g) * torch.tensor([20.0, 4.0, 1.0]) + torch.tensor([35.0, 0, 0]),
                       "size": torch.relu(torch.randn(B, N, 3, generator=g) + 2.0),
                       "angle": torch.tanh(torch.randn(B, N, 2, generator=g)),
                       "class": torch.randn(B, N, ncls, generator=g)})
    gt_box = torch.zeros(B, Mmax, 8)
    gt_onehot = torch.zeros(B, Mmax, ncls)
    targets = []
    for b, m in enumerate(counts):
        u, s = torch.rand(m, 3, generator=g), torch.rand(m, 3, generator=g)
        yaw = (torch.rand(m, generator=g) * 2 - 1) * 3.14159
        t = {"gt_center": torch.stack((5 + u[:, 0] * 65, -6 + u[:, 1] * 12, -1.5 + u[:, 2] * 3.5), -1),
             "gt_size": torch.stack((3.5 + s[:, 0] * 1.5, 1.6 + s[:, 1] * 0.6, 1.4 + s[:, 2] * 0.6), -1),
             "gt_angle": torch.stack((torch.sin(yaw), torch.cos(yaw)), -1),
             "gt_class": torch.eye(ncls)[torch.randint(0, ncls, (m,), generator=g)].reshape(m, ncls)}
        targets.append(t)
        gt_box[b, :m] = torch.cat((t["gt_center"], t["gt_size"], t["gt_angle"]), -1)
        gt_onehot[b, :m] = t["gt_class"]
    case = {"spec": spec, "cpu": layers, "targets": targets,
            "layers": [{k: v.to(DEV).clone() for k, v in l.items()} for l in layers],      # one allocation per tensor
            "gt_box": gt_box.to(DEV), "gt_onehot": gt_onehot.to(DEV),
            "gt_id": gt_onehot.argmax(-1).to(torch.int32).to(DEV),
            "counts": torch.tensor(counts, dtype=torch.int32, device=DEV),
            "sel": torch.ones(5, device=DEV),
            "weights": [CYCLE[l % 3] for l in range(L)]}
    return case


def _table(case, weights=None, grads=None, layers=None):
    from dpft_amd.training.loss import _layer_table
    layers = case["layers"] if layers is None else layers
    weights = case["weights"] if weights is None else weights
    tens = [tuple(l[k] for k in KEYS) for l in layers]
    return _layer_table(tens, weights, None if grads is None else [None if g is None else tuple(g[k] for k in KEYS) for g in grads])


def _cost_layers(case):
    from dpft_amd.hip.lib import lib, stream
    L, B, N, Mmax, ncls, _ = case["spec"]
    cost = torch.full((L, B, N, Mmax), float("nan"), device=DEV)
    tiled = torch.full((L * B,), -7, dtype=torch.int32, device=DEV)
    cw = (C.c_float * 5)(*COST_W)
    lib.call("dpft_match_cost_layers_f32", _table(case), L, case["gt_box"].data_ptr(), case["gt_id"].data_ptr(),
             case["counts"].data_ptr(), C.byref(cw), cost.data_ptr(), tiled.data_ptr(), B, N, Mmax, ncls, stream())
    return cost, tiled


def _cost_single(case, layer):
    from dpft_amd.hip.lib import lib, stream
    L, B, N, Mmax, ncls, _ = case["spec"]
    cost = torch.full((B, N, Mmax), float("nan"), device=DEV)
    cw = (C.c_float * 5)(*COST_W)
    lib.call("dpft_match_cost_f32", layer["class"].data_ptr(), layer["center"].data_ptr(), layer["size"].data_ptr(),
             layer["angle"].data_ptr(), case["gt_box"].data_ptr(), case["gt_id"].data_ptr(), case["counts"].data_ptr(),
             C.byref(cw), cost.data_ptr(), B, N, Mmax, ncls, stream())
    return cost


def _assign(cost, counts, samples, N, Mmax):
    from dpft_amd.hip.lib import lib, stream
    match = torch.full((samples, Mmax, 2), -9, dtype=torch.int32, device=DEV)
    matched = torch.full((samples,), -9, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    lib.call("dpft_lsap_batch_dev_f32", cost.data_ptr(), counts.data_ptr(), match.data_ptr(), matched.data_ptr(),
             status.data_ptr(), samples, N, Mmax, stream())
    assert int(status) == 0
    return match, matched


def _fwd_single(case, layer, match, matched):
    from dpft_amd.hip.lib import lib, stream
    L, B, N, Mmax, ncls, _ = case["spec"]
    scratch = torch.zeros(int(lib.dpft_set_loss_scratch_floats(B, N)), device=DEV)
    losses, total = torch.full((5,), float("nan"), device=DEV), torch.full((), float("nan"), device=DEV)
    w = (C.c_float * 5)(*W5)
    lib.call("dpft_set_loss_fwd_total_f32", layer["class"].data_ptr(), layer["center"].data_ptr(), layer["size"].data_ptr(),
             layer["angle"].data_ptr(), case["gt_box"].data_ptr(), case["gt_onehot"].data_ptr(), match.data_ptr(),
             matched.data_ptr(), C.byref(w), ALPHA, case["sel"].data_ptr(), scratch.data_ptr(), losses.data_ptr(),
             total.data_ptr(), B, N, Mmax, ncls, stream())
    return losses, total


def _fwd_layers(case, match, matched, scratch=None):
    from dpft_amd.hip.lib import lib, stream
    L, B, N, Mmax, ncls, _ = case["spec"]
    if scratch is None:
        scratch = torch.zeros(int(lib.dpft_set_loss_layers_scratch_floats(L, B, N)), device=DEV)
    losses = torch.full((L, 5), float("nan"), device=DEV)
    layer_totals, total = torch.full((L,), float("nan"), device=DEV), torch.full((), float("nan"), device=DEV)
    w = (C.c_float * 5)(*W5)
    lib.call("dpft_set_loss_layers_fwd_total_f32", _table(case), L, case["gt_box"].data_ptr(), case["gt_onehot"].data_ptr(),
             match.data_ptr(), matched.data_ptr(), C.byref(w), ALPHA, case["sel"].data_ptr(), scratch.data_ptr(),
             losses.data_ptr(), layer_totals.data_ptr(), total.data_ptr(), B, N, Mmax, ncls, stream())
    return losses, layer_totals, total


def _bwd_single(case, layer, match, matched, gout5):
    from dpft_amd.hip.lib import lib, stream
    L, B, N, Mmax, ncls, _ = case["spec"]
    grads = {k: torch.full_like(layer[k], float("nan")) for k in KEYS}
    w = (C.c_float * 5)(*W5)
    lib.call("dpft_set_loss_bwd_f32", layer["class"].data_ptr(), layer["center"].data_ptr(), layer["size"].data_ptr(),
             layer["angle"].data_ptr(), case["gt_box"].data_ptr(), case["gt_onehot"].data_ptr(), match.data_ptr(),
             matched.data_ptr(), C.byref(w), ALPHA, gout5.data_ptr(), grads["class"].data_ptr(), grads["center"].data_ptr(),
             grads["size"].data_ptr(), grads["angle"].data_ptr(), B, N, Mmax, ncls, stream())
    return grads


def _bwd_layers(case, match, matched, weights, gout=None):
    from dpft_amd.hip.lib import lib, stream
    L, B, N, Mmax, ncls, _ = case["spec"]
    grads = [{k: torch.full_like(l[k], float("nan")) for k in KEYS} for l in case["layers"]]
    w = (C.c_float * 5)(*W5)
    lib.call("dpft_set_loss_layers_bwd_f32", _table(case, weights, grads), L, case["gt_box"].data_ptr(),
             case["gt_onehot"].data_ptr(), match.data_ptr(), matched.data_ptr(), C.byref(w), ALPHA, case["sel"].data_ptr(),
             None if gout is None else gout.data_ptr(), B, N, Mmax, ncls, stream())
    return grads


@pytest.fixture(scope="module")
def cases():
    """Every case of the lattice with its layered cost and assignment, computed once and left unchanged."""
    out = []
    for spec in LATTICE:
        L, B, N, Mmax, ncls, _ = spec
        case = _make(spec)
        case["cost"], case["tiled"] = _cost_layers(case)
        match, matched = _assign(case["cost"], case["tiled"], L * B, N, Mmax)
        case["match"], case["matched"] = match.view(L, B, Mmax, 2), matched.view(L, B)
        out.append(case)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("k", range(len(LATTICE)), ids=IDS)
def test_layered_cost_is_the_single_output_cost_of_every_layer(cases, k):
    case = cases[k]
    L, B, N, Mmax, ncls, counts = case["spec"]
    assert case["tiled"].tolist() == list(counts) * L
    for l, layer in enumerate(case["layers"]):
        assert _same_bits(case["cost"][l], _cost_single(case, layer)), l
        for b, m in enumerate(counts):
            assert not bool(case["cost"][l, b, :, m:].any())
            assert bool(torch.isfinite(case["cost"][l, b]).all())


@pytest.mark.parametrize("k", range(len(LATTICE)), ids=IDS)
def test_layered_assignment_is_the_assignment_of_every_layer_alone(cases, k):
    from oracle import dprt_oracle as O
    case = cases[k]
    L, B, N, Mmax, ncls, counts = case["spec"]
    w = dict(zip(("total_class", "center", "size", "angle"), COST_W[:4]))
    for l in range(L):
        match, matched = _assign(case["cost"][l].contiguous(), case["counts"], B, N, Mmax)
        assert torch.equal(case["match"][l], match) and torch.equal(case["matched"][l], matched), l
        assert matched.tolist() == [min(N, m) for m in counts]
        if case["spec"] not in SMALL:
            continue
        for b, m in enumerate(counts):
            if m == 0:
                assert bool((match[b] == -1).all())
                continue
            i, j, _ = O.hungarian({n: v[b] for n, v in case["cpu"][l].items()}, case["targets"][b], w)
            n = int(matched[b])
            assert match[b, :n, 0].tolist() == i.tolist() and match[b, :n, 1].tolist() == j.tolist(), (l, b)


@pytest.mark.parametrize("k", range(len(LATTICE)), ids=IDS)
def test_layered_forward_rows_totals_and_scratch(cases, k):
    """losses[l] has the bits of the single-output forward on layer l.  layer_totals[l] = fp32(w_l) * (sum_k sel[k] * losses[l,k])
    is 5 products + 4 additions + 1 product = 10 fp32 roundings, total = their sum in layer order adds L - 1: against the fp64
    value of the same fp32 rows the bound is that count x 2^-24 x the (all non-negative) sum."""
    from dpft_amd.hip.lib import lib
    case = cases[k]
    L, B, N, Mmax, ncls, counts = case["spec"]
    match, matched = case["match"], case["matched"]
    scratch = torch.zeros(int(lib.dpft_set_loss_layers_scratch_floats(L, B, N)), device=DEV)
    losses, layer_totals, total = _fwd_layers(case, match, matched, scratch)
    for l, layer in enumerate(case["layers"]):
        single, single_total = _fwd_single(case, layer, match[l], matched[l])
        assert _same_bits(losses[l], single), l
        if case["weights"][l] == 1.0:
            assert _same_bits(layer_totals[l], single_total), l
    assert bool((losses >= 0).all()) and float(losses.sum()) > 0
    w32 = torch.tensor(case["weights"], dtype=torch.float32).double()
    ref_lt = w32 * (losses.double().cpu() * case["sel"].double().cpu()).sum(-1)
    u = 2.0 ** -24
    for l in range(L):
        print(f"layer {l}: total {float(layer_totals[l])!r} fp64 {float(ref_lt[l])!r}")
        assert abs(float(layer_totals[l]) - float(ref_lt[l])) <= 10 * u * float(ref_lt[l]), l
    print(f"total {float(total)!r} fp64 {float(ref_lt.sum())!r}")
    assert abs(float(total) - float(ref_lt.sum())) <= (10 + L - 1) * u * float(ref_lt.sum())
    # the scratch is left zero, and a second launch into it gives the same bits
    assert not bool(scratch.view(torch.int32).any())
    again = _fwd_layers(case, match, matched, scratch)
    for a, b in zip((losses, layer_totals, total), again):
        assert _same_bits(a, b)
    assert not bool(scratch.view(torch.int32).any())


@pytest.mark.parametrize("k", range(len(LATTICE)), ids=IDS)
def test_layered_gradient_is_the_single_output_gradient_of_every_layer(cases, k):
    case = cases[k]
    L, B, N, Mmax, ncls, counts = case["spec"]
    match, matched = case["match"], case["matched"]
    grads = _bwd_layers(case, match, matched, case["weights"])
    for l, layer in enumerate(case["layers"]):
        gout5 = torch.tensor(case["weights"][l], dtype=torch.float32, device=DEV) * case["sel"]
        single = _bwd_single(case, layer, match[l], matched[l], gout5)
        for key in KEYS:
            assert _same_bits(grads[l][key], single[key]), (l, key)
        if any(counts):
            assert bool(grads[l]["class"].any())
    # a device scalar gout = 3: the NULL form with every weight pre-multiplied in fp32
    three = torch.tensor(3.0, device=DEV)
    scaled = _bwd_layers(case, match, matched, case["weights"], gout=three)
    pre = [float(np.float32(w) * np.float32(3.0)) for w in case["weights"]]
    twin = _bwd_layers(case, match, matched, pre)
    for l in range(L):
        for key in KEYS:
            assert _same_bits(scaled[l][key], twin[l][key]), (l, key)


@pytest.mark.parametrize("k", range(len(LATTICE)), ids=IDS)
def test_layered_values_and_gradients_against_fp64_autograd(cases, k):
    case = cases[k]
    L, B, N, Mmax, ncls, counts = case["spec"]
    match, matched = case["match"].cpu(), case["matched"].cpu()
    leafs = [{n: v.double().clone().requires_grad_(True) for n, v in layer.items()} for layer in case["cpu"]]
    targets = [{n: v.double() for n, v in t.items()} for t in case["targets"]]
    matches = [[None if counts[b] == 0 else (match[l, b, :int(matched[l, b]), 0].long(), match[l, b, :int(matched[l, b]), 1].long())
                for b in range(B)] for l in range(L)]
    w32 = [float(np.float32(w)) for w in case["weights"]]
    ref_total, ref_losses, ref_lt = R.layered_total(leafs, targets, W, w32, matches)
    ref_total.backward()
    losses, layer_totals, total = _fwd_layers(case, case["match"], case["matched"])
    close(total, ref_total, rtol=1e-5, what="total")
    close(layer_totals, ref_lt, rtol=1e-5, what="layer totals")
    close(losses, ref_losses, rtol=1e-5, what="losses")
    grads = _bwd_layers(case, case["match"], case["matched"], case["weights"])
    for l in range(L):
        for key in KEYS:
            close(grads[l][key], leafs[l][key].grad, rtol=1e-4, what=f"layer {l} d/d{key}")


def _raw(name, *args):
    from dpft_amd.hip.lib import lib
    rc = getattr(lib.load(), name)(*args)
    return rc, lib.dpft_last_error().decode()


def test_refusals_return_a_message_and_launch_nothing(cases):
    from dpft_amd.hip.lib import lib, stream
    case = cases[1]
    L, B, N, Mmax, ncls, _ = case["spec"]
    cw, w = (C.c_float * 5)(*COST_W), (C.c_float * 5)(*W5)
    nan = float("nan")
    cost = torch.full((8, B, N, Mmax), nan, device=DEV)
    tiled = torch.full((8 * B,), -7, dtype=torch.int32, device=DEV)
    losses, lt, total = torch.full((8, 5), nan, device=DEV), torch.full((8,), nan, device=DEV), torch.full((), nan, device=DEV)
    scratch = torch.zeros(int(lib.dpft_set_loss_layers_scratch_floats(8, B, N)), device=DEV)
    packed = torch.full((8 * B * Mmax * 2 + 8 * B,), -9, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    grads = [{k: torch.full_like(l[k], nan) for k in KEYS} for l in case["layers"]]
    nine = [case["layers"][0]] * 9

    def half(table):
        table[1].dsize = None
        return table
    bad = [("0 layers", lambda: (_table(case), 0), r"0 layers, expected 1\.\.8"),
           ("9 layers", lambda: (_table(case, [1.0] * 9, layers=nine), 9), r"9 layers, expected 1\.\.8"),
           ("half a gradient quadruple", lambda: (half(_table(case, grads=grads)), L), r"layer 1 names 3 of its 4 gradient buffers"),
           ("negative weight", lambda: (_table(case, [1.0, -0.5]), L), r"layer 1 has weight -0\.5"),
           ("non-finite weight", lambda: (_table(case, [float("inf"), 1.0]), L), r"layer 0 has weight inf")]
    import re
    for what, make, pattern in bad:
        table, n = make()
        calls = [
            ("dpft_match_cost_layers_f32", (table, n, case["gt_box"].data_ptr(), case["gt_id"].data_ptr(), case["counts"].data_ptr(),
                                            C.byref(cw), cost.data_ptr(), tiled.data_ptr(), B, N, Mmax, ncls, stream())),
            ("dpft_set_loss_layers_fwd_total_f32", (table, n, case["gt_box"].data_ptr(), case["gt_onehot"].data_ptr(),
                                                    case["match"].data_ptr(), case["matched"].data_ptr(), C.byref(w), ALPHA,
                                                    case["sel"].data_ptr(), scratch.data_ptr(), losses.data_ptr(), lt.data_ptr(),
                                                    total.data_ptr(), B, N, Mmax, ncls, stream())),
            ("dpft_set_loss_layers_bwd_f32", (table, n, case["gt_box"].data_ptr(), case["gt_onehot"].data_ptr(),
                                              case["match"].data_ptr(), case["matched"].data_ptr(), C.byref(w), ALPHA,
                                              case["sel"].data_ptr(), None, B, N, Mmax, ncls, stream())),
            ("dpft_assign_loss_layers_dev_f32", (case["cost"].data_ptr(), case["tiled"].data_ptr(), packed.data_ptr(),
                                                 status.data_ptr(), table, n, case["gt_box"].data_ptr(),
                                                 case["gt_onehot"].data_ptr(), C.cast(w, C.c_void_p), ALPHA, case["sel"].data_ptr(),
                                                 scratch.data_ptr(), losses.data_ptr(), lt.data_ptr(), total.data_ptr(), B, N, Mmax,
                                                 ncls, stream())),
        ]
        for name, args in calls:
            rc, msg = _raw(name, *args)
            assert rc != 0 and re.search(pattern, msg), (what, name, rc, msg)
    torch.cuda.synchronize()
    # nothing was launched: every output still holds its fill, the scratch its zeros
    for t in (cost, losses, lt, total, *[g[k] for g in grads for k in KEYS]):
        assert bool(torch.isnan(t).all())
    assert bool((tiled == -7).all()) and bool((packed == -9).all()) and not bool(scratch.view(torch.int32).any())
    # a backward in which no layer names gradient buffers is refused as well
    rc, msg = _raw("dpft_set_loss_layers_bwd_f32", _table(case), L, case["gt_box"].data_ptr(), case["gt_onehot"].data_ptr(),
                   case["match"].data_ptr(), case["matched"].data_ptr(), C.byref(w), ALPHA, case["sel"].data_ptr(), None, B, N,
                   Mmax, ncls, stream())
    assert rc != 0 and "no layer names gradient buffers" in msg


def test_a_layer_without_gradient_buffers_is_left_out_of_the_backward(cases):
    case = cases[3]
    L = case["spec"][0]
    full = _bwd_layers(case, case["match"], case["matched"], case["weights"])
    from dpft_amd.hip.lib import lib, stream
    _, B, N, Mmax, ncls, _ = case["spec"]
    grads = [None if l == 2 else {k: torch.full_like(layer[k], float("nan")) for k in KEYS} for l, layer in enumerate(case["layers"])]
    w = (C.c_float * 5)(*W5)
    lib.call("dpft_set_loss_layers_bwd_f32", _table(case, grads=grads), L, case["gt_box"].data_ptr(), case["gt_onehot"].data_ptr(),
             case["match"].data_ptr(), case["matched"].data_ptr(), C.byref(w), ALPHA, case["sel"].data_ptr(), None, B, N, Mmax,
             ncls, stream())
    for l in range(L):
        if l != 2:
            for k in KEYS:
                assert _same_bits(grads[l][k], full[l][k])


@pytest.mark.parametrize("k", [1, 3], ids=[IDS[1], IDS[3]])
def test_host_and_device_assign_loss_entries_agree(cases, k):
    """dpft_assign_loss_layers_f32 (host assignment + one upload) and dpft_assign_loss_layers_dev_f32 from the same cost: the
    same packed table, losses, totals and gradients, bit for bit -- and those of the separate launches above."""
    from dpft_amd.hip.lib import lib, stream
    case = cases[k]
    L, B, N, Mmax, ncls, counts = case["spec"]
    n_match = L * B * Mmax * 2
    w = (C.c_float * 5)(*W5)
    res = {}
    for mode in ("dev", "host"):
        grads = [{key: torch.full_like(l[key], float("nan")) for key in KEYS} for l in case["layers"]]
        packed = torch.full((n_match + L * B,), -9, dtype=torch.int32, device=DEV)
        losses, lt, total = torch.empty((L, 5), device=DEV), torch.empty(L, device=DEV), torch.empty((), device=DEV)
        scratch = torch.zeros(int(lib.dpft_set_loss_layers_scratch_floats(L, B, N)), device=DEV)
        tail = (_table(case, grads=grads), L, case["gt_box"].data_ptr(), case["gt_onehot"].data_ptr(), C.cast(w, C.c_void_p), ALPHA,
                case["sel"].data_ptr(), scratch.data_ptr(), losses.data_ptr(), lt.data_ptr(), total.data_ptr(), B, N, Mmax, ncls,
                stream())
        if mode == "dev":
            status = torch.zeros(1, dtype=torch.int32, device=DEV)
            rc, msg = _raw("dpft_assign_loss_layers_dev_f32", case["cost"].data_ptr(), case["tiled"].data_ptr(), packed.data_ptr(),
                           status.data_ptr(), *tail)
        else:
            host = case["cost"].cpu().numpy()
            pin = torch.empty(n_match + L * B, dtype=torch.int32).pin_memory()
            cnt = np.asarray(counts, dtype=np.int32)
            rc, msg = _raw("dpft_assign_loss_layers_f32", host.ctypes.data, cnt.ctypes.data, pin.numpy().ctypes.data,
                           packed.data_ptr(), *tail)
        assert rc == 0, msg
        torch.cuda.synchronize()
        res[mode] = (packed, losses, lt, total, grads)
    for a, b in zip(res["dev"][:4], res["host"][:4]):
        assert _same_bits(a, b)
    assert torch.equal(res["dev"][0][:n_match].view(L, B, Mmax, 2), case["match"])
    assert torch.equal(res["dev"][0][n_match:].view(L, B), case["matched"])
    losses, lt, total = _fwd_layers(case, case["match"], case["matched"])
    assert _same_bits(res["dev"][1], losses) and _same_bits(res["dev"][2], lt) and _same_bits(res["dev"][3], total)
    ref = _bwd_layers(case, case["match"], case["matched"], case["weights"])
    for mode in res:
        for l in range(L):
            for key in KEYS:
                assert _same_bits(res[mode][4][l][key], ref[l][key]), (mode, l, key)


# ----------------------------------------------------------------------------------------------------------------------- Loss
AUX_W = [1.0, 0.5]


def _loss(on_device, aux_weights=None, giou=None):
    from dpft_amd.training.loss import Loss
    weights = dict(W) if giou is None else {**W, "giou": giou}
    loss = Loss.from_config({"anassigner": "HungarianAnassigner", "criterion": "SetCriterion", "loss_weights": weights,
                             "reduction": "mean"})
    loss.assign_on_device = on_device
    loss.aux_weights = aux_weights
    return loss


def _outputs(seed, B=2, N=12, ncls=3):
    g = torch.Generator().manual_seed(seed)
    out = {"class": torch.randn(B, N, ncls, generator=g), "center": torch.randn(B, N, 3, generator=g) * 2,
           "size": torch.rand(B, N, 3, generator=g) * 3 + 1, "angle": torch.randn(B, N, 2, generator=g)}
    return {k: v.to(DEV).requires_grad_(True) for k, v in out.items()}


def _labels(counts, seed, ncls=3):
    g = torch.Generator().manual_seed(seed)
    labels = []
    for m in counts:
        labels.append({"gt_center": (torch.randn(m, 3, generator=g) * 2).to(DEV), "gt_size": (torch.rand(m, 3, generator=g) * 3 + 1).to(DEV),
                       "gt_angle": torch.randn(m, 2, generator=g).to(DEV),
                       "gt_class": torch.eye(ncls)[torch.randint(0, ncls, (m,), generator=g)].to(DEV)})
    return labels


def _three(seed):
    """(final output, [iteration 0, iteration 1]) of a three-iteration decoder, every tensor a leaf."""
    return _outputs(seed), [_outputs(seed + 1), _outputs(seed + 2)]


def _plain(on_device, out, labels, giou=None):
    """A Loss without aux on one output: (total, losses, grads)."""
    loss = _loss(on_device, giou=giou)
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in out.items()}
    total, losses = loss(leaf, labels)
    total.backward()
    loss.check_assignment_status()
    return total.detach(), {k: v.detach() for k, v in losses.items()}, {k: v.grad for k, v in leaf.items()}


@pytest.mark.parametrize("on_device", [False, True], ids=["host-assignment", "device-assignment"])
@pytest.mark.parametrize("counts", [(3, 0), (1, 4)])
def test_loss_with_aux_outputs_is_the_plain_loss_on_every_output(on_device, counts):
    final, aux = _three(20)
    labels = _labels(counts, 70)
    loss = _loss(on_device, AUX_W)
    total, losses = loss({**final, "aux_outputs": aux}, labels)
    assert list(losses) == list(W) + ["aux_0", "aux_1"]
    assert loss.last_has_targets is True
    total.backward()
    loss.check_assignment_status()
    ref_total, ref_losses, ref_grads = _plain(on_device, final, labels)
    for k in W:
        assert _same_bits(losses[k], ref_losses[k]), k
    for k in final:
        assert _same_bits(final[k].grad, ref_grads[k]), k
    expect = ref_total.double()
    for i, wi in enumerate(AUX_W):                              # powers of two: the scaling is exact
        t_i, _, g_i = _plain(on_device, aux[i], labels)
        assert _same_bits(losses[f"aux_{i}"], t_i * wi), i
        for k in aux[i]:
            assert _same_bits(aux[i][k].grad, g_i[k] * wi), (i, k)
        expect = expect + float(t_i) * wi
    # total = the three layer totals added in layer order: 2 fp32 additions of non-negative numbers
    assert abs(float(total.detach()) - float(expect)) <= 2 * 2.0 ** -24 * float(expect)


def test_loss_with_aux_outputs_and_no_target_is_exactly_zero_with_all_keys():
    final, aux = _three(23)
    loss = _loss(True, AUX_W)
    total, losses = loss({**final, "aux_outputs": aux}, _labels((0, 0), 5))
    assert float(total.detach()) == 0.0 and loss.last_has_targets is False
    assert list(losses) == list(W) + ["aux_0", "aux_1"] and all(float(v.detach()) == 0.0 for v in losses.values())
    total.backward()


def test_zero_weight_leaves_the_iteration_out_of_the_launch(monkeypatch):
    from dpft_amd.hip.lib import lib
    layers_seen, orig = [], lib.call

    def recording(name, *args):
        if name == "dpft_match_cost_layers_f32":
            layers_seen.append(args[1])
        return orig(name, *args)
    monkeypatch.setattr(lib, "call", recording)
    final, aux = _three(26)
    labels = _labels((2, 3), 76)
    loss = _loss(True, [0.0, 0.5])
    total, losses = loss({**final, "aux_outputs": aux}, labels)
    total.backward()
    assert layers_seen == [2]
    assert float(losses["aux_0"]) == 0.0 and float(losses["aux_1"]) > 0.0
    assert all(aux[0][k].grad is None or not bool(aux[0][k].grad.any()) for k in aux[0])
    t_1, _, g_1 = _plain(True, aux[1], labels)
    assert _same_bits(losses["aux_1"], t_1 * 0.5)
    for k in aux[1]:
        assert _same_bits(aux[1][k].grad, g_1[k] * 0.5), k


def test_aux_weights_of_the_wrong_length_and_the_scipy_switch_are_refused(monkeypatch):
    final, aux = _three(29)
    labels = _labels((2, 3), 79)
    with pytest.raises(ValueError, match="aux_weights must be a list of 2 finite numbers"):
        _loss(True, [1.0])({**final, "aux_outputs": aux}, labels)
    with pytest.raises(ValueError, match="aux_weights must be a list of 2 finite numbers"):
        _loss(True, [1.0, -1.0])({**final, "aux_outputs": aux}, labels)
    monkeypatch.setenv("DPFT_LSAP_C", "0")
    with pytest.raises(ValueError, match="DPFT_LSAP_C=0"):
        _loss(False, AUX_W)({**final, "aux_outputs": aux}, labels)


def test_aux_outputs_without_aux_weights_run_todays_code(monkeypatch):
    from dpft_amd.hip.lib import lib
    names, orig = [], lib.call

    def recording(name, *args):
        names.append(name)
        return orig(name, *args)
    monkeypatch.setattr(lib, "call", recording)
    final, aux = _three(32)
    labels = _labels((2, 3), 82)
    total, losses = _loss(True)({**final, "aux_outputs": aux}, labels)
    total.backward()
    assert list(losses) == list(W) and not [n for n in names if "layers" in n]
    ref_total, _, ref_grads = _plain(True, final, labels)
    assert _same_bits(total, ref_total)
    for k in final:
        assert _same_bits(final[k].grad, ref_grads[k])
    assert all(v.grad is None for o in aux for v in o.values())


@pytest.mark.parametrize("on_device", [False, True], ids=["host-assignment", "device-assignment"])
def test_giou_term_stays_on_the_final_output(on_device, monkeypatch):
    from dpft_amd.hip.lib import lib
    names, orig = [], lib.call

    def recording(name, *args):
        names.append(name)
        return orig(name, *args)
    final, aux = _three(35)
    labels = _labels((2, 3), 85)
    loss = _loss(on_device, AUX_W, giou=2.0)
    with monkeypatch.context() as m:
        m.setattr(lib, "call", recording)
        total, losses = loss({**final, "aux_outputs": aux}, labels)
        total.backward()
    assert [n for n in names if "giou_loss" in n] == ["dpft_giou_loss_fwd_f32", "dpft_giou_loss_bwd_f32"]      # once each
    assert list(losses) == list(W) + ["giou", "aux_0", "aux_1"]
    ref_total, ref_losses, ref_grads = _plain(on_device, final, labels, giou=2.0)
    five_total, _, five_grads = _plain(on_device, final, labels)
    assert _same_bits(losses["giou"], ref_losses["giou"]) and float(losses["giou"]) > 0
    # its share of the final gradient: what the giou-only Loss adds to the five-term gradient, the same bits here
    aux_only = _loss(on_device, AUX_W)
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in final.items()}
    aux_only({**leaf, "aux_outputs": [{k: v.detach() for k, v in o.items()} for o in aux]}, labels)[0].backward()
    for k in final:
        assert _same_bits(leaf[k].grad, five_grads[k]), k
        assert _same_bits(final[k].grad, ref_grads[k]), k
    # the aux iterations carry no GIoU share
    for i, wi in enumerate(AUX_W):
        _, _, g_i = _plain(on_device, aux[i], labels)
        for k in aux[i]:
            assert _same_bits(aux[i][k].grad, g_i[k] * wi), (i, k)


@pytest.mark.parametrize("giou", [None, 2.0], ids=["five-terms", "with-giou"])
def test_backward_into_named_buffers_of_all_layers(giou):
    final, aux = _three(38)
    labels = _labels((2, 3), 88)
    order = ("center", "size", "angle", "class")
    inputs = {**final, "aux_outputs": aux}
    # autograd
    loss = _loss(True, AUX_W, giou=giou)
    loss(inputs, labels)[0].backward()
    want = [o[k].grad.clone() for o in [final, *aux] for k in order]
    # (a) buffers named in advance: the forward's C call launches the gradient into them, backward_into has nothing left to do
    bufs = [torch.full_like(o[k], float("nan")) for o in [final, *aux] for k in order]
    loss.fused_grad_targets = tuple(bufs)
    total, _ = loss(inputs, labels)
    for b, g in zip(bufs, want):
        assert _same_bits(b, g)
    assert loss.__dict__["_bwd_written"] is not None and loss.backward_into(total, *bufs)
    # (b) buffers not named in advance: backward_into launches the layered gradient
    loss.fused_grad_targets = None
    total, _ = loss(inputs, labels)
    late = [torch.full_like(b, float("nan")) for b in bufs]
    assert loss.backward_into(total, *late)
    for b, g in zip(late, want):
        assert _same_bits(b, g)
    # (c) under no_grad nothing is written into named buffers
    untouched = [torch.full_like(b, float("nan")) for b in bufs]
    loss.fused_grad_targets = tuple(untouched)
    with torch.no_grad():
        loss(inputs, labels)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(b).all()) for b in untouched)
    assert loss.__dict__.get("_bwd_written") is None
    # four buffers alone do not fit a three-output forward
    loss.fused_grad_targets = None
    total, _ = loss(inputs, labels)
    with pytest.raises(ValueError, match="12|3 decoder outputs"):
        loss.backward_into(total, *late[:4])
