"""tests/aux_loss_ref.py (the fp64 restatement of the deep-supervision total) against the oracle: on random outputs -- the
generator of tests/test_gpu_model.py::test_loss_and_matcher_match_oracle at N = 40 -- the layered total equals
sum_l weight_l * O.loss_forward(out_l, targets, w)[0] with O.hungarian per layer.  CPU only."""
import pytest
import torch

from oracle import dprt_oracle as O
from tests import aux_loss_ref as R

B, N, L = 3, 40, 3
LAYER_W = (1.0, 0.5, 0.3)


def _case():
    from dpft_amd.configs import load_config
    from dpft_amd.synthetic import make_labels
    g = torch.Generator().manual_seed(5)
    outs = []
    for _ in range(L):
        out = {"center": torch.randn(B, N, 3, generator=g) * torch.tensor([20.0, 4.0, 1.0]) + torch.tensor([35.0, 0, 0]),
               "size": torch.relu(torch.randn(B, N, 3, generator=g) + 2.0),
               "angle": torch.tanh(torch.randn(B, N, 2, generator=g)),
               "class": torch.randn(B, N, 2, generator=g)}
        outs.append({k: v.double() for k, v in out.items()})
    labels = make_labels(B, seed=3)
    labels[1] = {k: v[:0] for k, v in labels[1].items()}            # a sample without objects
    labels = [{k: v.double() for k, v in l.items()} for l in labels]
    return outs, labels, dict(load_config("kradar")["train"]["loss_weights"])


@pytest.fixture(scope="module")
def case():
    outs, labels, w = _case()
    matches, costs = [], []
    for out in outs:
        per = []
        for b, lab in enumerate(labels):
            if lab["gt_class"].shape[0] == 0:
                per.append(None)
                continue
            i, j, C = O.hungarian({k: v[b] for k, v in out.items()}, lab, w)
            per.append((i, j))
            costs.append(C.numpy())
        matches.append(per)
    return outs, labels, w, matches, costs


def test_inputs_have_one_clear_best_assignment(case):
    """The condition under which fixed indices mean something, on the oracle's cost matrices alone: best and second-best
    assignment totals differ by more than 1e-6 relative in every one of them."""
    *_, costs = case
    assert len(costs) == L * (B - 1)
    gaps = [R.second_best_gap(C) for C in costs]
    print("relative gaps best / second best:", ["%.2e" % g for g in gaps])
    assert min(gaps) > 1e-6, gaps


def test_second_best_gap_on_a_matrix_with_known_totals():
    import numpy as np
    C = np.array([[1.0, 2.0], [2.0, 1.0], [5.0, 5.0]])           # best 2 (pairs 0-0, 1-1); second 4 (0-1, 1-0)
    assert R.second_best_gap(C) == pytest.approx(1.0)
    assert R.second_best_gap(np.array([[1.0, 1.0], [1.0, 1.0]])) == 0.0


def test_cost_restatement_gives_the_oracles_matrices(case):
    outs, labels, w, _, costs = case
    k = 0
    for out in outs:
        for b, lab in enumerate(labels):
            if lab["gt_class"].shape[0] == 0:
                continue
            o = {n: v[b] for n, v in out.items()}
            yaw = lambda a: torch.atan2(a[..., 0], a[..., 1])
            giou = O.giou3d_yaw(o["center"], o["size"], yaw(o["angle"]), lab["gt_center"], lab["gt_size"], yaw(lab["gt_angle"]))
            torch.testing.assert_close(R.cost_matrix(o, lab, w, giou.double()), torch.from_numpy(costs[k]), rtol=1e-12, atol=1e-12)
            k += 1


def test_layered_total_is_the_weighted_sum_of_the_oracles_totals(case):
    outs, labels, w, matches, _ = case
    total, losses, layer_totals = R.layered_total(outs, labels, w, LAYER_W, matches)
    ref_total = 0.0
    for l, (out, lw) in enumerate(zip(outs, LAYER_W)):
        t, terms = O.loss_forward(out, labels, w)
        ref_total = ref_total + lw * t
        torch.testing.assert_close(layer_totals[l], lw * t, rtol=1e-12, atol=0)
        for k, name in enumerate(R.TERMS):
            torch.testing.assert_close(losses[l, k], terms[name], rtol=1e-12, atol=1e-15)
    torch.testing.assert_close(total, ref_total, rtol=1e-12, atol=0)


def test_layered_gradient_is_the_weighted_gradient_of_each_layer(case):
    outs, labels, w, matches, _ = case
    leafs = [{k: v.clone().requires_grad_(True) for k, v in out.items()} for out in outs]
    R.layered_total(leafs, labels, w, LAYER_W, matches)[0].backward()
    for out, leaf, lw in zip(outs, leafs, LAYER_W):
        ref = {k: v.clone().requires_grad_(True) for k, v in out.items()}
        O.loss_forward(ref, labels, w)[0].backward()
        for k in ref:
            torch.testing.assert_close(leaf[k].grad, lw * ref[k].grad, rtol=1e-10, atol=1e-15)
