"""fp64 restatement of the deep-supervision loss (train.aux_loss): the layered total
    total = sum_l weight_l * sum_k w_k / B * sum_b term_k(out_l[b], targets[b], match_l[b])
over L supervised decoder outputs that share their targets, each with its own assignment.  Written from the formulas in
DESIGN.md 3 (focal loss with the raw-logit p_t, alpha 0.75, gamma 2; L1 means over the matched pairs), independent of the
oracle's code: tests/test_aux_loss_ref.py holds it to ``oracle.dprt_oracle.loss_forward`` / ``hungarian``.  With the
assignments fixed it is differentiable, so fp64 autograd through it is the yardstick of the layered gradient kernel."""
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

TERMS = ("total_class", "object_class", "center", "size", "angle")
ALPHA, GAMMA = 0.75, 2.0


def _focal(x, t):
    ce = torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    pt = x * t + (1 - x) * (1 - t)                      # raw logits, as the reference has it
    return (ALPHA * t + (1 - ALPHA) * (1 - t)) * ce * (1 - pt) ** GAMMA


def sample_terms(out: Dict[str, torch.Tensor], tgt: Dict[str, torch.Tensor], i: torch.Tensor, j: torch.Tensor):
    """The five unweighted criterion terms of one sample for the pairs (i[k], j[k])."""
    x = out["class"]
    N, C = x.shape
    M = int(j.numel())
    one_hot = torch.zeros(N, C, dtype=x.dtype)
    one_hot[:, 0] = 1.0
    one_hot[i] = tgt["gt_class"].to(x.dtype)[:M]        # the k-th matched query takes the k-th target row
    terms = {"total_class": _focal(x, one_hot).sum() / N / M * N,
             "object_class": _focal(x[i], tgt["gt_class"].to(x.dtype)[j]).sum() / M / M * N}
    for k in ("center", "size", "angle"):
        terms[k] = (out[k][i] - tgt["gt_" + k].to(x.dtype)[j]).abs().mean()
    return terms


def cost_matrix(out, tgt, w, giou) -> torch.Tensor:
    """The matcher's (N, M) cost of one sample; ``giou`` (N, M) comes from the caller (the oracle's yaw-box GIoU3D)."""
    ids = tgt["gt_class"].argmax(-1)
    l1 = lambda k: (out[k][:, None, :] - tgt["gt_" + k][None, :, :]).abs().sum(-1)
    return -w["total_class"] * out["class"][:, ids] + w["center"] * l1("center") + w["size"] * l1("size") \
        + w["angle"] * l1("angle") - giou


def second_best_gap(cost: np.ndarray) -> float:
    """(second-best total - best total) / |best total| of a linear sum assignment problem: the best assignment that differs
    from the optimum drops at least one of its pairs, so it is the cheapest optimum with one optimal pair forbidden."""
    from scipy.optimize import linear_sum_assignment
    cost = np.asarray(cost, dtype=np.float64)
    i, j = linear_sum_assignment(cost)
    best = cost[i, j].sum()
    big = np.abs(cost).sum() + 1.0
    second = np.inf
    for a, b in zip(i, j):
        c = cost.copy()
        c[a, b] = big
        ii, jj = linear_sum_assignment(c)
        second = min(second, c[ii, jj].sum())
    return float((second - best) / max(abs(best), 1e-300))


def layered_total(outs: Sequence[Dict[str, torch.Tensor]], targets: List[Dict[str, torch.Tensor]], w: Dict[str, float],
                  layer_weights: Sequence[float], matches: Sequence[Sequence[Tuple[torch.Tensor, torch.Tensor]]]):
    """-> (total, losses (L, 5 in TERMS order, weighted batch means without the layer weight), layer_totals (L)).
    matches[l][b] = (i, j) int64 or None for a sample without targets."""
    B = len(targets)
    dtype = outs[0]["class"].dtype
    rows, totals = [], []
    for out, lw, match in zip(outs, layer_weights, matches):
        acc = {k: torch.zeros((), dtype=dtype) for k in TERMS}
        for b, tgt in enumerate(targets):
            if match[b] is None:
                continue
            terms = sample_terms({k: v[b] for k, v in out.items()}, tgt, *match[b])
            for k in TERMS:
                acc[k] = acc[k] + terms[k] * w.get(k, 0.0) / B
        rows.append(torch.stack([acc[k] for k in TERMS]))
        totals.append(lw * sum(acc[k] for k in TERMS if k in w))
    return sum(totals), torch.stack(rows), torch.stack(totals)
