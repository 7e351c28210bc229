"""CPU checks of the criterion's GIoU3D term: the fp64 restatement the GPU tests compare against (tests/giou_loss_ref.py)
against the oracle's GIoU and against central differences, the two C entries' boundary, and the configuration of ``Loss``."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import dprt_oracle as O
from tests import giou_loss_ref as R


def _oracle_parts(p):
    """(oracle GIoU, evol, v1, v2) of a lattice pair, the enclosing volume from the oracle's own corners."""
    ce, sz, an, gce, gsz, gan = R.tensors(p)
    ya, yg = torch.atan2(an[0], an[1]).reshape(1), torch.atan2(gan[0], gan[1]).reshape(1)
    g = float(O.giou3d_yaw(ce[None], sz[None], ya, gce[None], gsz[None], yg)[0, 0])
    corners = torch.cat((O.box_corners(ce[None], sz[None], ya)[0], O.box_corners(gce[None], gsz[None], yg)[0]), 0)
    evol = float((corners.max(0).values - corners.min(0).values).prod())
    return g, evol, float(sz.prod()), float(gsz.prod())


def test_lattice_has_every_named_class_and_the_random_pairs():
    names = [p["name"] for p in R.NAMED]
    assert names == ["partial_overlap", "disjoint_bev", "disjoint_z_only", "pred_inside_target", "target_inside_pred",
                     "eight_vertices", "unnormalised_angle", "zero_angle", "negative_size", "tiny_size"]
    assert len(R.LATTICE) == len(R.NAMED) + R.N_RANDOM and R.N_RANDOM >= 64
    for p in R.LATTICE:                                       # every value is an fp32 number
        for k in ("center", "size", "angle", "g_center", "g_size", "g_angle"):
            assert np.array_equal(p[k], p[k].astype(np.float32).astype(np.float64))
    by = {p["name"]: p for p in R.NAMED}
    parts = {}
    R.pair_value_and_grad(by["eight_vertices"], parts)
    assert parts["vertices"] == 8
    R.pair_value_and_grad(by["disjoint_bev"], parts)
    assert parts["vertices"] == 0 and parts["vol"] == 0.0
    R.pair_value_and_grad(by["disjoint_z_only"], parts)
    assert parts["vertices"] >= 3 and parts["vol"] == 0.0     # the rectangles overlap, the z ranges do not
    R.pair_value_and_grad(by["pred_inside_target"], parts)
    assert abs(parts["vol"] - parts["v1"]) < 1e-12
    R.pair_value_and_grad(by["target_inside_pred"], parts)
    assert abs(parts["vol"] - parts["v2"]) < 1e-12


def test_helper_equals_the_oracle_where_boxes_overlap_and_the_textbook_value_where_not():
    n_overlap = n_disjoint = 0
    for p in R.LATTICE:
        parts = {}
        G, grad = R.pair_value_and_grad(p, parts)
        if p["name"] in R.INVALID:
            assert G == -1.0 and not grad.any(), p["name"]
            continue
        g_oracle, evol, v1, v2 = _oracle_parts(p)
        if parts["vol"] > 0:
            n_overlap += 1
            assert abs(G - g_oracle) <= 1e-12, (p["name"], G, g_oracle)
        else:
            n_disjoint += 1
            assert g_oracle == -1.0                           # the reference's quirk, kept in the matcher
            assert abs(G - (-(evol - v1 - v2) / evol)) <= 1e-12, (p["name"], G)
            assert -1.0 < G < 0.0
    assert n_overlap >= 20 and n_disjoint >= 20, (n_overlap, n_disjoint)


def test_autograd_agrees_with_central_differences_on_every_valid_pair():
    """Conditions the lattice, not the kernel: away from the min / max ties (where no gradient is defined) autograd and
    central differences (h = 1e-6) agree to 1e-6 * max|grad|.  No pair is excluded."""
    worst = 0.0
    for p in R.LATTICE:
        if p["name"] in R.INVALID:
            continue
        _, grad = R.pair_value_and_grad(p)
        num = R.pair_numeric_grad(p, h=1e-6)
        scale = np.abs(grad).max()
        assert scale > 0, p["name"]
        ratio = np.abs(num - grad).max() / scale
        worst = max(worst, ratio)
        assert ratio <= 1e-6, (p["name"], ratio)
    print(f"worst |numeric - autograd| / max|grad| over the lattice: {worst:.2e}")


def test_zero_angle_has_no_angle_gradient_and_the_unnormalised_one_is_tangential():
    by = {p["name"]: p for p in R.NAMED}
    _, g0 = R.pair_value_and_grad(by["zero_angle"])
    assert g0[6] == 0.0 and g0[7] == 0.0 and np.abs(g0[:6]).max() > 0
    p = by["unnormalised_angle"]
    _, g = R.pair_value_and_grad(p)
    s, c = p["angle"]
    assert abs(g[6] * s + g[7] * c) <= 1e-12 * np.abs(g[6:]).max()      # yaw does not depend on the radius


def test_the_entries_are_exported_have_signatures_and_reject_bad_arguments():
    from dpft_amd.hip.lib import SIGNATURES, lib
    dll = lib.load()
    p = [C.c_void_p(4096 * (i + 1)) for i in range(12)]      # never read: validation comes before any launch
    err = lambda: lib.dpft_last_error().decode()
    for name in ("dpft_giou_loss_fwd_f32", "dpft_giou_loss_bwd_f32"):
        assert name in SIGNATURES and hasattr(dll, name)

    def fwd(center=p[0], term=p[7], total_in=p[6], total_out=p[8], w=1.0, B=2, N=4, Mmax=3):
        return lib.dpft_giou_loss_fwd_f32(center, p[1], p[2], p[3], p[4], p[5], w, total_in, term, total_out, None, B, N, Mmax, None)

    def bwd(center=p[0], dangle=p[9], w=1.0, B=2, N=4, Mmax=3):
        return lib.dpft_giou_loss_bwd_f32(center, p[1], p[2], p[3], p[4], p[5], w, None, p[7], p[8], dangle, 0, B, N, Mmax, None)

    for call, entry in ((fwd, "giou_loss_fwd: "), (bwd, "giou_loss_bwd: ")):
        assert call(center=None) == -1 and err().startswith(entry) and "null" in err()
        for bad in ({"B": 0}, {"N": -1}, {"Mmax": 0}):
            assert call(**bad) == -1 and err().startswith(entry) and "sizes" in err(), bad
        for w in (float("nan"), float("inf"), -0.5):
            assert call(w=w) == -1 and err().startswith(entry) and "weight" in err(), w
    assert fwd(term=None) == -1 and err().startswith("giou_loss_fwd: ")
    assert fwd(total_in=None) == -1 and "come together" in err()
    assert fwd(total_out=None) == -1 and "come together" in err()
    assert bwd(dangle=None) == -1 and err().startswith("giou_loss_bwd: ")


def _config(weights):
    return {"anassigner": "HungarianAnassigner", "criterion": "SetCriterion", "loss_weights": weights, "reduction": "mean"}


BASE = {"total_class": 1.0, "object_class": 0.0, "center": 1.0, "size": 1.0, "angle": 1.0}


def test_loss_accepts_the_key_and_refuses_bad_weights():
    from dpft_amd.training.loss import Loss
    loss = Loss.from_config(_config({**BASE, "giou": 2.0}))
    assert loss.loss_weights["giou"] == 2.0 and "giou" not in Loss._TERMS
    assert Loss.from_config(_config({**BASE, "giou": 0})).loss_weights["giou"] == 0      # weight 0 still logs the term
    assert Loss.from_config(_config(BASE)).loss_weights == BASE
    for bad in (-1, float("nan"), float("inf"), -0.0 - 1e-9, "2", None, True):
        with pytest.raises(ValueError, match="giou"):
            Loss.from_config(_config({**BASE, "giou": bad}))
    assert math.isfinite(loss.loss_weights["giou"])


def test_the_term_has_no_eager_path():
    """With the key configured and the fused path unavailable (here: CPU tensors) the loss says so; it does not fall into
    the eager loop's KeyError.  Without the key the eager path runs as before."""
    from dpft_amd.training.loss import Loss
    g = torch.Generator().manual_seed(0)
    out = {"class": torch.randn(1, 4, 3, generator=g), "center": torch.randn(1, 4, 3, generator=g),
           "size": torch.rand(1, 4, 3, generator=g) + 1, "angle": torch.randn(1, 4, 2, generator=g)}
    labels = [{"gt_center": torch.randn(2, 3, generator=g), "gt_size": torch.rand(2, 3, generator=g) + 1,
               "gt_angle": torch.randn(2, 2, generator=g), "gt_class": torch.eye(3)[:2]}]
    with pytest.raises(ValueError, match="fused path only"):
        Loss.from_config(_config({**BASE, "giou": 2.0}))(out, labels)
    cuda_only = Loss.from_config(_config({**BASE, "giou": 2.0}))
    cuda_only.reduction = "sum"
    with pytest.raises(ValueError, match="fused path only"):
        cuda_only(out, labels)
