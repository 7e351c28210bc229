"""Gradient clipping by global norm, the parts that need no GPU: the fp64 yardstick of tests/test_gpu_grad_clip.py against
torch, the ``train.clip_grad_norm`` config key, the trainer's eager path (any optimizer but FusedAdamW: torch's clip_grad_norm_
between reducer.finish() and optimizer.step()) on one rank and on two gloo ranks."""
import copy
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import grad_clip_ref as R


def test_reference_recurrence_matches_torch_fp64():
    """The helper (everything in fp64, kernel_scalars=False) against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW run in
    fp64 on the CPU over three steps: norm, coefficient, parameters and both moments.  Both sides are fp64 and differ only in
    operation order, so 1e-10 relative, element by element.  One tensor has no gradient in the second step (it sits out and
    keeps its own step count); some gradient elements are exactly 0; the coefficient is below 1 in every step."""
    g = torch.Generator().manual_seed(17)
    numels = [3, 257, 5, 1000, 1]
    lr, betas, eps, wd, max_norm = 1e-2, (0.9, 0.999), 1e-8, 1e-2, 0.75
    params = [torch.nn.Parameter(torch.randn(n, generator=g).double()) for n in numels]
    opt = torch.optim.AdamW(params, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    ref = R.AdamWRef([p.detach().numpy() for p in params], lr=lr, betas=betas, eps=eps, weight_decay=wd, kernel_scalars=False)
    for step in range(3):
        grads = []
        for i, (p, n) in enumerate(zip(params, numels)):
            if step == 1 and i == 2:
                p.grad = None
                grads.append(None)
                continue
            gr = torch.randn(n, generator=g).float()                 # fp32 values, as the kernels see them
            gr[torch.rand(n, generator=g) < 0.1] = 0.0
            p.grad = gr.double()
            grads.append(gr.numpy().copy())
        norm_t = float(torch.nn.utils.clip_grad_norm_([p for p in params if p.grad is not None], max_norm))
        opt.step()
        norm, coef = ref.clipped_step(grads, max_norm)
        assert coef < 1.0
        assert abs(norm - norm_t) <= 1e-10 * norm_t
        got_coef = [float(p.grad[j] / float(gr[j])) for p, gr in zip(params, grads) if gr is not None
                    for j in np.flatnonzero(gr)[:1]]
        assert all(abs(c - coef) <= 1e-10 * coef for c in got_coef), (got_coef, coef)
    for i, p in enumerate(params):
        st = opt.state[p]
        assert float(st["step"]) == ref.steps[i] == (2 if i == 2 else 3)
        for name, got, want in (("p", p.detach(), ref.P[i]), ("m", st["exp_avg"], ref.M[i]), ("v", st["exp_avg_sq"], ref.V[i])):
            np.testing.assert_allclose(want, got.numpy(), rtol=1e-10, atol=0, err_msg=f"tensor {i} {name}")


def test_reference_unclipped_step_carries_no_gradient_error_term():
    """coef == 1 is the plain AdamW step: same values as a step without a coefficient, and the bound has no E_g part."""
    p0 = [np.linspace(-1, 1, 7)]
    gr = [np.float32(np.linspace(0.5, -0.25, 7))]
    a, b = R.AdamWRef(p0), R.AdamWRef(p0)
    norm, coef = a.clipped_step(gr, 1e30)
    b.step(gr)
    assert coef == 1.0 and abs(norm - float(np.sqrt((gr[0].astype(np.float64) ** 2).sum()))) < 1e-15
    assert np.array_equal(a.P[0], b.P[0]) and np.array_equal(a.EP[0], b.EP[0])
    assert R.norm_coef([np.float32([np.nan, 1.0])], 0.1)[1] != R.norm_coef([np.float32([np.nan, 1.0])], 0.1)[1]      # NaN
    assert R.norm_coef([np.float32([np.inf, 1.0])], 0.1) == (float("inf"), 0.0)
    assert R.ulps_f32(np.float32(1.0) + np.float32(2.0 ** -23), 1.0) == 1.0


def test_clip_grad_norm_config_forms():
    from dpft_amd.training.trainer import parse_clip_grad_norm
    assert parse_clip_grad_norm(0.1) == (0.1, "propagate")
    assert parse_clip_grad_norm(2) == (2.0, "propagate")
    assert parse_clip_grad_norm({"max_norm": 0.1}) == (0.1, "propagate")
    assert parse_clip_grad_norm({"max_norm": 5.0, "nonfinite": "skip"}) == (5.0, "skip")
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), None, "0.1", True, [0.1], {}, {"nonfinite": "skip"},
                {"max_norm": 0.0}, {"max_norm": "1"}, {"max_norm": 1.0, "nonfinite": "ignore"},
                {"max_norm": 1.0, "norm_type": 2}):
        with pytest.raises(ValueError, match="clip_grad_norm"):
            parse_clip_grad_norm(bad)


class _Tiny(torch.nn.Module):
    """Every parameter receives a gradient (a parameter without one is decayed by torch.optim.AdamW only if it has a .grad:
    the reducer gives every parameter a zero-filled bucket view, a bare loop does not)."""

    def __init__(self):
        super().__init__()
        self.net = torch.nn.Sequential(torch.nn.Linear(6, 16), torch.nn.Tanh(), torch.nn.Linear(16, 4))

    def forward(self, data):
        return {"y": self.net(data["x"])}


class _TinyLoss(torch.nn.Module):
    def forward(self, output, labels):
        loss = 50.0 * ((output["y"] - labels[0]["y"]) ** 2).sum(1).mean()      # (scaled: the norm is far above max_norm)
        return loss, {"mse": loss}


_tiny_loss = _TinyLoss()


def _tiny_config(clip):
    from dpft_amd.configs import load_config
    cfg = copy.deepcopy(load_config("kradar"))
    cfg["train"]["optimizer"] = {"name": "AdamW", "lr": 1e-2}
    cfg["evaluate"] = {}
    if clip is not None:
        cfg["train"]["clip_grad_norm"] = clip
    return cfg


def _tiny_trainer(clip):
    from dpft_amd.training.trainer import DataParallelTrainer
    torch.manual_seed(0)
    tr = DataParallelTrainer(_Tiny(), _tiny_config(clip), "cpu")
    tr.loss_fn = _TinyLoss()
    return tr


def _tiny_data(rank=None):
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(8, 6, generator=g), torch.randn(8, 4, generator=g)
    if rank is not None:
        x, y = x[rank * 4:(rank + 1) * 4], y[rank * 4:(rank + 1) * 4]
    return {"x": x}, [{"y": y}]


def test_trainer_rejects_a_bad_clip_key_at_construction():
    from dpft_amd.training.trainer import DataParallelTrainer
    with pytest.raises(ValueError, match="clip_grad_norm"):
        DataParallelTrainer(_Tiny(), _tiny_config(-0.1), "cpu")
    cfg = _tiny_config(0.1)
    cfg["train"]["clip_grad_norm"] = None                                   # present but empty: not "absent"
    with pytest.raises(ValueError, match="clip_grad_norm"):
        DataParallelTrainer(_Tiny(), cfg, "cpu")
    tr = _tiny_trainer(None)
    assert tr.clip is None and tr.last_grad_norm is None


def test_cpu_trainer_step_with_the_key_equals_a_hand_clipped_step():
    """The eager path: with the key set and an optimizer that is not FusedAdamW the trainer clips the reducer's final gradients
    with torch.nn.utils.clip_grad_norm_ between finish() and step().  Two steps equal clip_grad_norm_ + torch.optim.AdamW by
    hand on a twin; ``last_grad_norm`` is the norm before clipping; without the key the same trainer takes another step."""
    max_norm = 0.1
    tr = _tiny_trainer({"max_norm": max_norm})
    assert isinstance(tr.optimizer, torch.optim.AdamW) and tr.clip == (max_norm, "propagate")
    assert float(tr.last_grad_norm) == 0.0                                   # no backward yet
    torch.manual_seed(0)
    twin = _Tiny()
    opt = torch.optim.AdamW(twin.parameters(), lr=1e-2)
    plain = _tiny_trainer(None)
    data, labels = _tiny_data()
    for _ in range(2):
        loss, losses = tr.train_step(data, labels)
        plain.train_step(data, labels)
        opt.zero_grad(set_to_none=True)
        want_loss, _ = _tiny_loss(twin(data), labels)
        want_loss.backward()
        norm = torch.nn.utils.clip_grad_norm_(twin.parameters(), max_norm)
        opt.step()
        assert float(norm) > 10 * max_norm                                  # the clip bites
        torch.testing.assert_close(loss, want_loss.detach(), rtol=1e-6, atol=0)
        torch.testing.assert_close(tr.last_grad_norm, norm, rtol=1e-6, atol=0)
        assert set(losses) == {"mse"}
    for (n, p), q, r in zip(tr.model.named_parameters(), twin.parameters(), plain.model.parameters()):
        torch.testing.assert_close(p.detach(), q.detach(), rtol=1e-6, atol=1e-7, msg=lambda m: f"{n}: {m}")
    assert plain.last_grad_norm is None
    assert any(not torch.equal(p.detach(), r.detach()) for p, r in zip(tr.model.parameters(), plain.model.parameters()))


def test_cpu_trainer_skip_mode_drops_a_step_with_a_nan_norm():
    tr = _tiny_trainer({"max_norm": 0.1, "nonfinite": "skip"})
    data, labels = _tiny_data()
    tr.train_step(data, labels)
    before = [p.detach().clone() for p in tr.model.parameters()]
    bad = {"x": data["x"].clone()}
    bad["x"][0, 0] = float("inf")                                           # a positive (infinite) loss with NaN gradients
    tr.train_step(bad, labels)
    assert not bool(torch.isfinite(tr.last_grad_norm)) and tr.nonfinite_steps() == 1
    for p, b in zip(tr.model.parameters(), before):
        assert torch.equal(p.detach(), b)
    tr.train_step(data, labels)
    assert tr.nonfinite_steps() == 1 and bool(torch.isfinite(tr.last_grad_norm))
    assert all(not torch.equal(p.detach(), b) for p, b in zip(tr.model.parameters(), before))


def test_epoch_loop_logs_grad_norm_only_with_the_key(tmp_path):
    """train_one_epoch adds grad_norm to the step's scalars (averaged, logged as train/grad_norm) only when the key is set."""
    class _Writer:
        def __init__(self):
            self.tags = []

        def add_scalar(self, tag, value, step):
            self.tags.append(tag)
    data, labels = _tiny_data()
    loader = [(data, labels), (data, labels)]
    for clip, has in ((0.1, True), (None, False)):
        tr = _tiny_trainer(clip)
        tr.logging = "epoch"
        w = _Writer()
        means = tr.train_one_epoch(0, loader, w)
        assert ("grad_norm" in means) == has and ("train/grad_norm" in w.tags) == has
        assert {"train/loss", "train/loss_mse"} <= set(w.tags)
        if has:
            assert means["grad_norm"] > 1.0


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    tr = _tiny_trainer(0.1)
    assert tr.collective and tr.world == world
    data, labels = _tiny_data(rank)                          # each rank its own shard
    norms = []
    for _ in range(2):
        tr.train_step(data, labels)
        norms.append(float(tr.last_grad_norm))
    q.put((rank, norms, [p.detach().numpy().copy() for p in tr.model.parameters()]))
    dist.destroy_process_group()


def test_two_ranks_report_the_same_norm_and_end_with_equal_parameters():
    """World-2 gloo: the norm is taken after reducer.finish(), on gradients both ranks hold identically, so no new collective is
    needed -- both ranks report the same ``last_grad_norm`` (the global batch's: the one-rank trainer's on the whole batch) and
    end the steps with equal parameters."""
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {r: (n, ps) for r, n, ps in (q.get(timeout=120) for _ in range(world))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][0] == res[1][0] and all(n > 1.0 for n in res[0][0])
    for a, b in zip(res[0][1], res[1][1]):
        assert np.array_equal(a, b)
    one = _tiny_trainer(0.1)
    data, labels = _tiny_data()
    one.train_step(data, labels)
    assert abs(float(one.last_grad_norm) - res[0][0][0]) <= 1e-5 * res[0][0][0]
