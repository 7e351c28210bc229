"""EMA of the weights, the parts that need no GPU: the fp64 yardstick of tests/test_gpu_ema.py against torch, the ``train.ema``
config key, and the trainer's eager path (any optimizer but FusedAdamW: ``torch._foreach_lerp_`` after optimizer.step())."""
import copy
import os

import numpy as np
import pytest
import torch

from tests import ema_ref as R


def test_reference_matches_torch_ema_rule_in_fp64():
    """The recurrence of the helper against torch.optim.swa_utils.get_ema_multi_avg_fn (Tensor.lerp_ where the installed torch
    lacks it) on fp64 tensors over 30 steps.  decay = 1 - 2^-5 is exact in fp32 and so is 1 - decay, so both sides use the same
    weight; both are fp64 and differ only in operation order: 1e-12 relative, element by element."""
    decay = 1.0 - 2.0 ** -5
    w = R.weight(decay)
    assert float(w) == 2.0 ** -5 == 1.0 - decay
    g = torch.Generator().manual_seed(21)
    numels = [3, 257, 1]
    ema = [torch.randn(n, generator=g, dtype=torch.float64) for n in numels]
    e0 = [e.numpy().copy() for e in ema]
    try:
        from torch.optim.swa_utils import get_ema_multi_avg_fn
        fn = get_ema_multi_avg_fn(decay)
    except ImportError:
        def fn(avg, cur, _):
            for a, c in zip(avg, cur):
                a.lerp_(c, 1.0 - decay)
    ps = []
    for step in range(30):
        cur = [torch.randn(n, generator=g, dtype=torch.float64) for n in numels]
        ps.append([c.numpy().copy() for c in cur])
        fn(ema, cur, step)
    for i in range(len(numels)):
        want = R.trajectory(e0[i], [p[i] for p in ps], [w] * 30)[-1]
        np.testing.assert_allclose(ema[i].numpy(), want, rtol=1e-12, atol=0)


def test_reference_weight_and_warmup_schedule():
    """w is the once-rounded fp32 of 1 - d_eff with the decay rounded to fp32 first; the warm-up is min(decay, (1 + n) / (10 + n))
    on the tensor's own count; a tensor that sits out keeps its value in the recurrence."""
    assert R.weight(0.99) == np.float32(1.0 - float(np.float32(0.99)))
    assert R.weight(0.99) != np.float32(0.01)                     # (1 - fp32(0.99) is not fp32(0.01))
    assert R.decay_eff(0.999, True, 1) == 2.0 / 11.0 and R.decay_eff(0.999, True, 5) == 6.0 / 15.0
    assert R.decay_eff(0.5, True, 100) == 0.5 and R.decay_eff(0.5, True, 8) == 0.5 and R.decay_eff(0.5, True, 7) == 8.0 / 17.0
    assert R.weight(0.0) == np.float32(1.0)
    e = R.trajectory(np.float32([1.0, -2.0]), [np.float32([3.0, 0.0])] * 3, [np.float32(0.5), None, np.float32(0.25)])
    assert np.array_equal(e[0], [2.0, -1.0]) and np.array_equal(e[1], e[0]) and np.array_equal(e[2], [2.25, -0.75])
    assert np.array_equal(R.one_step_bound([1.0, -8.0], [-2.0, 4.0]), [2.0 ** -20, 2.0 ** -18])


def test_ema_config_forms():
    from dpft_amd.training.trainer import parse_ema
    full = {"decay": 0.99, "warmup": False, "validate": True, "save": True}
    assert parse_ema(0.99) == full
    assert parse_ema(0) == dict(full, decay=0.0)
    assert parse_ema({"decay": 0.99}) == full
    assert parse_ema({"decay": 0.5, "warmup": True, "validate": False, "save": False}) == \
        {"decay": 0.5, "warmup": True, "validate": False, "save": False}
    for bad in (1, 1.0, -0.1, 1.5, 0.99999999, 10 ** 400, -10 ** 400, {"decay": 10 ** 400}, float("inf"), float("nan"), None, "0.99", True, [0.99], {}, {"warmup": True},
                {"decay": 1.0}, {"decay": "0.9"}, {"decay": 0.9, "warmup": 1}, {"decay": 0.9, "validate": "yes"},
                {"decay": 0.9, "save": None}, {"decay": 0.9, "interval": 2}):
        with pytest.raises(ValueError, match="train.ema"):
            parse_ema(bad)


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.net = torch.nn.Sequential(torch.nn.Linear(6, 16), torch.nn.Tanh(), torch.nn.Linear(16, 4))

    def forward(self, data):
        return {"y": self.net(data["x"])}


class _TinyLoss(torch.nn.Module):
    """scale * mse: a scale of 0 gives a loss that is not positive, i.e. a step that does not step."""

    def forward(self, output, labels):
        loss = labels[0]["scale"] * ((output["y"] - labels[0]["y"]) ** 2).sum(1).mean()
        return loss, {"mse": loss}


def _tiny_trainer(ema):
    from dpft_amd.configs import load_config
    from dpft_amd.training.trainer import DataParallelTrainer
    cfg = copy.deepcopy(load_config("kradar"))
    cfg["train"]["optimizer"] = {"name": "AdamW", "lr": 1e-2}
    cfg["evaluate"] = {}
    if ema is not None:
        cfg["train"]["ema"] = ema
    torch.manual_seed(0)
    tr = DataParallelTrainer(_Tiny(), cfg, "cpu")
    tr.loss_fn = _TinyLoss()
    return tr


def _tiny_data(scale=1.0):
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(8, 6, generator=g), torch.randn(8, 4, generator=g)
    return {"x": x}, [{"y": y, "scale": torch.tensor(scale)}]


def test_trainer_rejects_a_bad_ema_key_at_construction_and_is_inert_without_it():
    with pytest.raises(ValueError, match="train.ema"):
        _tiny_trainer(1.0)
    with pytest.raises(ValueError, match="train.ema"):
        _tiny_trainer({"decay": 0.9, "every": 2})
    tr = _tiny_trainer(None)
    assert tr.ema is None and tr.ema_parameters() is None
    before = [p.detach().clone() for p in tr.model.parameters()]
    with tr.ema_weights():                                                  # a no-op
        assert all(torch.equal(p.detach(), b) for p, b in zip(tr.model.parameters(), before))


@pytest.mark.parametrize("ema", [0.99, {"decay": 0.9, "warmup": True}])
def test_eager_ema_follows_the_reference_and_sits_out_a_step_that_did_not_step(ema):
    """The eager path (torch.optim.AdamW on the CPU): after every step that stepped each EMA element is the fp64 one-step rule of
    its former value and the new parameter, with the kernel's fp32 weight of the step's own count, inside the one-step bound
    (torch's lerp_ evaluates p - (p - e) (1 - w) for w >= 0.5: four roundings, (6 (1 - w) + 1) u max <= 4 u max, inside the same
    bound).  The third step has a loss of zero: it does not step, and the EMA and its warm-up count stay where they were."""
    tr = _tiny_trainer(ema)
    assert isinstance(tr.optimizer, torch.optim.AdamW)
    decay, warmup = (ema, False) if not isinstance(ema, dict) else (ema["decay"], ema["warmup"])
    params = list(tr.model.parameters())
    assert all(torch.equal(e, p.detach()) for e, p in zip(tr.ema_parameters(), params))      # seeded with the weights
    own = 0
    for step, scale in enumerate((50.0, 50.0, 0.0, 50.0, 50.0)):
        e_old = [e.clone() for e in tr.ema_parameters()]
        p_old = [p.detach().clone() for p in params]
        tr.train_step(*_tiny_data(scale))
        if scale == 0.0:
            assert all(torch.equal(p.detach(), b) for p, b in zip(params, p_old))
            assert all(torch.equal(e, b) for e, b in zip(tr.ema_parameters(), e_old))
            continue
        own += 1
        w = R.weight(decay, warmup, own)
        for e, eo, p, po in zip(tr.ema_parameters(), e_old, params, p_old):
            assert not torch.equal(p.detach(), po)
            want = R.one_step(eo.numpy(), p.detach().numpy(), w)
            err = np.abs(e.double().numpy() - want)
            assert (err <= R.one_step_bound(eo.numpy(), p.detach().numpy())).all(), (step, float(err.max()))
            assert not torch.equal(e, eo)
    assert own == 4 and (w == R.weight(0.9, True, 4) if warmup else w == R.weight(0.99))


def test_eager_ema_state_round_trips():
    """EagerEMA keeps its averages and warm-up counts outside the optimizer: state_dict() / load_state_dict() carry them to a
    resumed run, which then takes the same next step bit for bit; a state of another shape is refused."""
    from dpft_amd.training.trainer import EagerEMA
    cfg = {"decay": 0.9, "warmup": True}
    a, b = _tiny_trainer(cfg), _tiny_trainer(cfg)
    for _ in range(3):
        a.train_step(*_tiny_data(50.0))
    state = a._ema_eager.state_dict()
    assert state["counts"] == [3] * len(state["ema"])
    b.model.load_state_dict(a.model.state_dict())
    b.optimizer.load_state_dict(copy.deepcopy(a.optimizer.state_dict()))      # (torch may alias the tensors it is given)
    b._ema_eager.load_state_dict(state)
    a.train_step(*_tiny_data(50.0))
    assert all(torch.equal(s, e) for s, e in zip(state["ema"], b.ema_parameters()))      # (the state is a copy, not a view)
    b.train_step(*_tiny_data(50.0))
    assert b._ema_eager.counts == a._ema_eager.counts == [4] * len(state["ema"])
    assert all(torch.equal(x, y) for x, y in zip(a.ema_parameters(), b.ema_parameters()))
    with pytest.raises(ValueError, match="EagerEMA"):
        EagerEMA([torch.nn.Parameter(torch.zeros(3))], 0.9).load_state_dict(state)


def test_eager_ema_weights_context_validation_and_checkpoint(tmp_path):
    """ema_weights() swaps the EMA in and back bit for bit (also when the body raises); validate_one_epoch returns the loss under
    the EMA unless ``validate`` is false; save_checkpoint writes ``<stem>_ema<ext>`` with the EMA as parameters next to the
    plain file unless ``save`` is false, and dpft_amd.models.load reads it."""
    from dpft_amd.hip.lib import weights_generation
    from dpft_amd.models import load
    tr = _tiny_trainer(0.9)
    off = _tiny_trainer({"decay": 0.9, "validate": False, "save": False})
    data, labels = _tiny_data(50.0)
    for _ in range(3):
        tr.train_step(data, labels)
        off.train_step(data, labels)
    params = list(tr.model.parameters())
    live = [p.detach().clone() for p in params]
    ema = [e.clone() for e in tr.ema_parameters()]
    assert all(not torch.equal(a, b) for a, b in zip(live, ema))
    gen = weights_generation()
    with pytest.raises(RuntimeError, match="inside"):
        with tr.ema_weights():
            assert all(torch.equal(p.detach(), e) for p, e in zip(params, ema))
            assert all(torch.equal(e, l) for e, l in zip(tr.ema_parameters(), live))
            tr.model.eval()
            ema_loss = float(tr.loss_fn(tr.model(data), labels)[0].detach())
            raise RuntimeError("inside")
    assert weights_generation() == gen + 2
    assert all(torch.equal(p.detach(), l) for p, l in zip(params, live))
    assert all(torch.equal(e, b) for e, b in zip(tr.ema_parameters(), ema))
    live_loss = float(tr.loss_fn(tr.model(data), labels)[0].detach())
    assert ema_loss != live_loss
    assert tr.validate_one_epoch(0, [(data, labels)])["loss"] == ema_loss
    assert off.validate_one_epoch(0, [(data, labels)])["loss"] == live_loss      # the twin took the same steps
    assert all(torch.equal(p.detach(), l) for p, l in zip(params, live))
    path = str(tmp_path / "t_checkpoint_0003.pt")
    tr.save_checkpoint(path)
    off.save_checkpoint(str(tmp_path / "u_checkpoint_0003.pt"))
    assert sorted(os.listdir(tmp_path)) == ["t_checkpoint_0003.pt", "t_checkpoint_0003_ema.pt", "u_checkpoint_0003.pt"]
    plain, epoch, stamp = load(path)
    shipped, epoch_e, stamp_e = load(str(tmp_path / "t_checkpoint_0003_ema.pt"))
    assert (epoch, stamp) == (epoch_e, stamp_e) == (3, "t")
    assert all(torch.equal(q.detach(), l) for q, l in zip(plain.parameters(), live))
    assert all(torch.equal(q.detach(), e) for q, e in zip(shipped.parameters(), ema))
    assert all(torch.equal(p.detach(), l) for p, l in zip(params, live))
