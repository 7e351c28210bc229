"""Host side of deep supervision (train.aux_loss): the configuration parser, the decoding of the assignment status word for a
later layer, IMPFusion.return_aux off by default, and Loss refusing aux outputs off the device.  CPU only."""
import math
from collections import OrderedDict

import pytest
import torch
from torch import nn

from dpft_amd.training.trainer import parse_aux_loss


@pytest.mark.parametrize("value, i_iter, expected", [
    (True, 4, [1.0, 1.0, 1.0]),
    (0.5, 4, [0.5, 0.5, 0.5]),
    (2, 2, [2.0]),
    (0, 3, [0.0, 0.0]),
    ({"weights": 0.25}, 4, [0.25, 0.25, 0.25]),
    ({"weights": [1.0, 0.5, 0]}, 4, [1.0, 0.5, 0.0]),
    ({"weights": (0.1,)}, 2, [0.1]),
])
def test_parse_aux_loss_accepts(value, i_iter, expected):
    got = parse_aux_loss(value, i_iter)
    assert got == expected and all(type(x) is float for x in got)


@pytest.mark.parametrize("value, i_iter", [
    (False, 4), (None, 4), ("on", 4), (-1.0, 4), (math.nan, 4), (math.inf, 4), ([1.0, 1.0, 1.0], 4),
    ({"weights": [1.0, 1.0]}, 4), ({"weights": [1.0, 1.0, 1.0, 1.0]}, 4), ({"weights": [1.0, -0.5, 1.0]}, 4),
    ({"weights": [1.0, math.inf, 1.0]}, 4), ({"weights": [1.0, True, 1.0]}, 4), ({"weights": True}, 4),
    ({"weights": -2}, 4), ({"weights": "1"}, 4), ({"weight": 1.0}, 4), ({"weights": 1.0, "extra": 0}, 4), ({}, 4),
])
def test_parse_aux_loss_refuses_and_says_what_it_expected(value, i_iter):
    with pytest.raises(ValueError, match=r"train\.aux_loss: expected true, a finite number >= 0, or \{'weights'.*3 finite numbers"):
        parse_aux_loss(value, i_iter)


@pytest.mark.parametrize("value", [True, 1.0, {"weights": [1.0]}])
def test_parse_aux_loss_refuses_a_one_iteration_decoder(value):
    with pytest.raises(ValueError, match="i_iter = 1.*no intermediate output"):
        parse_aux_loss(value, 1)


def test_status_word_of_a_later_layer_names_output_and_sample():
    from dpft_amd.training.loss import Loss
    d = Loss.describe_assignment_status
    # as before without a batch size
    assert d(1 + 3) == "matcher: cost matrix of sample 3 contains invalid numeric entries"
    assert d(0x10000 + 2) == "matcher: cost matrix of sample 2 is infeasible"
    # B = 4: pseudo-sample l * B + b
    assert d(1 + 2, 4) == "matcher: cost matrix of sample 2 of the final output contains invalid numeric entries"
    assert d(1 + 2 * 4 + 3, 4) == "matcher: cost matrix of sample 3 of iteration 1 contains invalid numeric entries"
    assert d(0x10000 + 3 * 4 + 0, 4) == "matcher: cost matrix of sample 0 of iteration 2 is infeasible"
    assert d(0x20000 + 1 * 4 + 1, 4) == "matcher: cost matrix of sample 1 of iteration 0 has more targets than the packed width"
    # an iteration with weight 0 is left out of the launch: launched layer 2 is iteration 2 when iteration 1 was dropped
    assert d(1 + 2 * 4 + 1, 4, (0, 1, 3)) == "matcher: cost matrix of sample 1 of iteration 2 contains invalid numeric entries"


class _Head(nn.Module):
    def forward(self, query, out):
        return OrderedDict(center=out["center"] + query[..., :3].mean(), size=query[..., :3], angle=query[..., :2],
                           **{"class": query[..., :2] + out["center"].sum()})


def _fuser(monkeypatch, i_iter=3):
    """IMPFusion's eager loop on the CPU with the fusion layers stubbed out (they have no CPU path): what is under test is which
    head outputs the decoder hands out."""
    from dpft_amd.models.fusers.mpfusion import IMPFusion, MPFusion
    monkeypatch.setattr(MPFusion, "forward", lambda self, query, *a, **k: query * 1.5)
    fuser = IMPFusion(i_iter=i_iter, m_views=1, d_model=8, d_ffn=16, n_queries=5, n_levels=[1], n_heads=[1], n_points=[1],
                      head=_Head())
    B = 2
    args = dict(batch=[OrderedDict(p0=torch.zeros(B, 4, 4, 8))], shape=[torch.tensor([[4.0, 4.0]] * B)],
                projection=[(torch.zeros(B, 4, 4), torch.eye(3, 4).repeat(B, 1, 1))], out=OrderedDict(center=torch.rand(B, 5, 3)),
                has_transformation=[False])
    return fuser, args


def test_return_aux_is_off_by_default_and_eval_returns_no_extra_key(monkeypatch):
    from dpft_amd.models.fusers.mpfusion import IMPFusion
    assert IMPFusion.return_aux is False
    fuser, args = _fuser(monkeypatch)
    assert fuser.return_aux is False and "return_aux" not in fuser.__dict__
    keys = ["center", "size", "angle", "class"]
    assert list(fuser.train()(**args)) == keys
    fuser.eval()
    with torch.no_grad():
        assert list(fuser(**args)) == keys
        fuser.return_aux = True
        assert list(fuser(**args)) == keys                        # eval without grad mode: never


def test_return_aux_hands_out_every_intermediate_iteration(monkeypatch):
    fuser, args = _fuser(monkeypatch, i_iter=3)
    plain = fuser.train()(**args)
    fuser.return_aux = True
    out = fuser(**args)
    assert list(out) == ["center", "size", "angle", "class", "aux_outputs"]
    aux = out["aux_outputs"]
    assert len(aux) == 2 and all(list(o) == ["center", "size", "angle", "class"] for o in aux)
    for k in plain:
        assert torch.equal(out[k], plain[k])
    # iteration 0 first: its centres are the start centres moved once, the final ones moved three times
    assert not torch.equal(aux[0]["center"], aux[1]["center"]) and not torch.equal(aux[1]["center"], out["center"])
    assert torch.equal(aux[0]["size"] * 1.5, aux[1]["size"])
    fuser.eval()
    assert "aux_outputs" in fuser(**args)                          # eval under grad mode: the training kernels' path


def test_loss_on_the_cpu_ignores_or_refuses_aux_outputs(monkeypatch):
    from dpft_amd.synthetic import make_labels
    from dpft_amd.training.loss import Loss
    loss = Loss.from_config({"anassigner": "HungarianAnassigner", "criterion": "SetCriterion", "reduction": "mean",
                             "loss_weights": {"total_class": 1.0, "object_class": 1.0, "center": 1.0, "size": 1.0, "angle": 1.0}})
    assert loss.aux_weights is None
    g = torch.Generator().manual_seed(0)

    def outputs():
        return {"center": torch.randn(2, 6, 3, generator=g) * 10, "size": torch.rand(2, 6, 3, generator=g) + 1,
                "angle": torch.randn(2, 6, 2, generator=g), "class": torch.randn(2, 6, 2, generator=g)}
    final, labels = outputs(), make_labels(2, seed=1, max_boxes=3)
    # (the matcher's GIoU is a HIP kernel: the eager criterion is replaced by a recorder of what reaches it)
    seen = []
    monkeypatch.setattr(loss, "forward_eager", lambda inputs, targets: seen.append(inputs) or (torch.zeros(()), {}))
    loss(final, labels)
    loss({**final, "aux_outputs": [outputs()]}, labels)
    assert [list(s) for s in seen] == [["center", "size", "angle", "class"]] * 2
    assert all(seen[1][k] is final[k] for k in final)
    loss.aux_weights = [1.0]
    with pytest.raises(ValueError, match="fused path only"):
        loss({**final, "aux_outputs": [outputs()]}, labels)
