"""EMA of the weights inside the fused AdamW step: dpft_adamw_ema_f32 and dpft_swap_f32 through FusedAdamW.set_ema / swap_ema /
ema_parameters and the trainer's ``train.ema`` key, against the fp64 reference of tests/ema_ref.py (vetted against torch in
tests/test_ema_host.py).

The tensors are those of the AdamW edge test (tests/test_gpu_grad_clip.py): ends on a CHUNK = 16384 boundary, one short of it
and one past it, two chunks + 7, moment (and so EMA) offsets of every residue mod 4, one parameter that is a view at storage
offset 1 (4-byte aligned only) -- plus one channels-last 4-D parameter, whose flat slice is in khwc order."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import ema_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
ADAM_NUMELS = [3, 16384, 5, 16385, 1, 16383, 4, 32775]
KHWC_SHAPE = (8, 4, 3, 3)
HYPER = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
N_TENSORS = len(ADAM_NUMELS) + 1


def _params(seed):
    """Parameters on the device: the edge tensors (numel 16385 is a view at storage offset 1) and the channels-last one."""
    g = torch.Generator().manual_seed(seed)
    params = []
    for n in ADAM_NUMELS:
        init = torch.randn(n, generator=g)
        if n == 16385:
            p = torch.nn.Parameter(torch.empty(n + 1, device=DEV)[1:])
            assert p.data_ptr() % 16 == 4
        else:
            p = torch.nn.Parameter(torch.empty(n, device=DEV))
        p.data.copy_(init)
        params.append(p)
    w = torch.randn(KHWC_SHAPE, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    params.append(torch.nn.Parameter(w))
    assert not params[-1].is_contiguous()
    return params


def _grads(g, scale=1.0):
    """Random gradients (CPU, fp32), one per parameter, in the parameter's shape."""
    return [torch.randn(n, generator=g) * scale for n in ADAM_NUMELS] + [torch.randn(KHWC_SHAPE, generator=g) * scale]


def _set_grads(params, grads):
    for p, gr in zip(params, grads):
        if gr is None:
            p.grad = None
        elif p.dim() == 4:
            p.grad = gr.to(DEV).contiguous(memory_format=torch.channels_last)
        else:
            p.grad = gr.to(DEV)


def _cpu(ts):
    torch.cuda.synchronize()
    return [t.detach().cpu().clone() for t in ts]


def _state(opt, params):
    sd = opt.state_dict()["state"]
    return [(float(sd[i]["step"]), sd[i]["exp_avg"].detach().cpu().clone(), sd[i]["exp_avg_sq"].detach().cpu().clone())
            for i in range(len(params))]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _two_groups(params):
    from dpft_amd.training.optimizer import FusedAdamW
    return FusedAdamW([{"params": params[:4]}, {"params": params[4:], "lr": 3e-3}], **HYPER)


@pytest.mark.parametrize("decay,warmup", [(0.99, False), (0.999, True)])
def test_one_step_against_fp64(decay, warmup):
    """Two parameter groups, five steps; tensor 2 (numel 5) has no gradient in the first two.  After every step each EMA element
    is within 4 * 2^-23 * max(|e_old|, |p_new|) of the fp64 rule applied to the device's own e_old and p_new with the kernel's
    fp32 weight (tests/ema_ref.py: three fp32 roundings, (4 w + 1) * 2^-24 max, a factor below 2 of slack for contraction either
    way).  The tensor without a gradient keeps its EMA bit for bit; with warm-up its later weights follow ITS count."""
    params = _params(1)
    opt = _two_groups(params)
    opt.set_ema(decay, warmup=warmup)
    assert _same(_cpu(opt.ema_parameters()), _cpu(params))                  # seeded with the weights (tables built on demand)
    g = torch.Generator().manual_seed(2)
    own = [0] * N_TENSORS
    for step in range(5):
        grads = _grads(g)
        if step < 2:
            grads[2] = None
        _set_grads(params, grads)
        e_old = _cpu(opt.ema_parameters())
        p_old = _cpu(params)
        opt.step()
        e_new, p_new = _cpu(opt.ema_parameters()), _cpu(params)
        for i in range(N_TENSORS):
            if grads[i] is None:
                assert torch.equal(e_new[i], e_old[i]) and torch.equal(p_new[i], p_old[i])
                continue
            own[i] += 1
            w = R.weight(decay, warmup, own[i])
            want = R.one_step(e_old[i].numpy(), p_new[i].numpy(), w)
            err = np.abs(e_new[i].double().numpy() - want)
            bound = R.one_step_bound(e_old[i].numpy(), p_new[i].numpy())
            print(f"step {step} tensor {i} own {own[i]} w {w!r}: max err / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
            assert (err <= bound).all(), (step, i, int((err > bound).sum()), float(err.max()))
            assert not torch.equal(e_new[i], e_old[i]) and not torch.equal(p_new[i], p_old[i])
    assert own[2] == 3 and own[0] == 5
    if warmup:
        assert R.weight(decay, True, 3) != R.weight(decay, True, 5)          # (tensor 2's last weight was its own)


def test_trajectory_stays_within_the_sum_of_the_local_bounds():
    """25 steps; the fp64 recurrence is driven by the device's parameter trajectory.  The lerp is a contraction (0 <= w <= 1), so
    the local errors add and do not grow: after step k the device EMA is within k one-step bounds, each taken with the largest
    max(|e|, |p|) the element has seen so far -- at most 25 x the one-step bound at the end."""
    from dpft_amd.training.optimizer import FusedAdamW
    decay = 0.9
    params = _params(3)
    opt = FusedAdamW(params, **HYPER)
    opt.set_ema(decay)
    w = R.weight(decay)
    e64 = [e.double().numpy() for e in _cpu(opt.ema_parameters())]
    seen = [np.abs(e) for e in e64]
    g = torch.Generator().manual_seed(4)
    worst = 0.0
    for k in range(1, 26):
        _set_grads(params, _grads(g))
        opt.step()
        p_new, e_dev = _cpu(params), _cpu(opt.ema_parameters())
        for i in range(N_TENSORS):
            seen[i] = np.maximum(seen[i], np.maximum(np.abs(p_new[i].double().numpy()), np.abs(e_dev[i].double().numpy())))
            e64[i] = R.one_step(e64[i], p_new[i].numpy(), w)
            err = np.abs(e_dev[i].double().numpy() - e64[i])
            bound = k * 4.0 * 2.0 ** -23 * seen[i]
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (k, i, float(err.max()))
    print(f"trajectory: worst err / (k x one-step bound) = {worst:.4f}")


@pytest.mark.parametrize("clip", [None, 0.5])
def test_ema_has_no_effect_on_the_update(clip):
    """p, m, v and the per-parameter step counts after five steps (tensor 2 without a gradient in two of them) are bit-equal
    between an optimizer with the EMA on and one without, unclipped and with set_clip(0.5)."""
    pa, pb = _params(5), _params(5)
    oa, ob = _two_groups(pa), _two_groups(pb)
    ob.set_ema(0.99, warmup=True)
    for o in (oa, ob):
        if clip is not None:
            o.set_clip(clip)
    g = torch.Generator().manual_seed(6)
    for step in range(5):
        grads = _grads(g)
        if step in (1, 2):
            grads[2] = None
        _set_grads(pa, grads)
        _set_grads(pb, grads)
        oa.step()
        ob.step()
    assert _same(_cpu(pa), _cpu(pb))
    for i, ((sa, ma, va), (sb, mb, vb)) in enumerate(zip(_state(oa, pa), _state(ob, pb))):
        assert sa == sb == (3.0 if i == 2 else 5.0) and torch.equal(ma, mb) and torch.equal(va, vb)
    assert not _same(_cpu(ob.ema_parameters()), _cpu(pb))
    if clip is not None:
        assert float(ob.last_grad_norm()) > clip                            # the clip bit


def test_closed_gate_and_skipped_step_leave_the_ema_alone_and_coef_one_is_the_unclipped_ema():
    """A closed gate (set_gate of a zero loss) and a NaN gradient under "nonfinite": "skip" leave the EMA bit-equal (and p, and the
    own step counts the warm-up reads).  max_norm = 1e30 (coef == 1.0f) with the EMA on equals the unclipped EMA run bit for bit."""
    pa, pb = _params(7), _params(7)
    oa, ob = _two_groups(pa), _two_groups(pb)
    oa.set_ema(0.99, warmup=True)
    ob.set_ema(0.99, warmup=True)
    ob.set_clip(1e30, nonfinite="skip")
    g = torch.Generator().manual_seed(8)
    for step in range(4):
        grads = _grads(g)
        _set_grads(pa, grads)
        _set_grads(pb, grads)
        oa.step()
        ob.step()
        if step == 1:                                                       # b alone: a closed gate, then a step with a NaN gradient
            e_old, p_old = _cpu(ob.ema_parameters()), _cpu(pb)
            ob.set_gate(torch.tensor(0.0, device=DEV))
            ob.step()
            assert _same(_cpu(ob.ema_parameters()), e_old) and _same(_cpu(pb), p_old)
            bad = _grads(g)
            bad[7][20000] = float("nan")
            _set_grads(pb, bad)
            ob.step()
            assert ob.nonfinite_steps() == 1
            assert _same(_cpu(ob.ema_parameters()), e_old) and _same(_cpu(pb), p_old)
    assert float(ob._clip_record.view(torch.float32)[1]) == 1.0
    assert _same(_cpu(pa), _cpu(pb)) and _same(_cpu(oa.ema_parameters()), _cpu(ob.ema_parameters()))
    assert not _same(_cpu(oa.ema_parameters()), _cpu(pa))
    assert [s for s, _, _ in _state(ob, pb)] == [4.0] * N_TENSORS


def test_swap_exchanges_weights_and_ema_in_place():
    """After swap_ema() the parameters hold the former EMA bits and the EMA the former parameter bits; a second swap restores
    both.  A tensor that lost its gradient after the tables were built (it has no chunk row any more) is swapped too.  The
    parameters keep their storage, and weights_generation() advances by one per swap."""
    from dpft_amd.hip.lib import weights_generation
    params = _params(9)
    opt = _two_groups(params)
    opt.set_ema(0.9)
    g = torch.Generator().manual_seed(10)
    for _ in range(2):
        _set_grads(params, _grads(g))
        opt.step()
    grads = _grads(g)
    grads[3] = None                                                         # numel 16385, the misaligned view: trained, sits out now
    _set_grads(params, grads)
    opt.step()                                                              # (the tables are rebuilt without rows for it)
    p0, e0 = _cpu(params), _cpu(opt.ema_parameters())
    assert all(not torch.equal(a, b) for a, b in zip(p0, e0))
    ptrs = [p.data_ptr() for p in params]
    gen = weights_generation()
    opt.swap_ema()
    assert weights_generation() == gen + 1
    assert _same(_cpu(params), e0) and _same(_cpu(opt.ema_parameters()), p0)
    opt.swap_ema()
    assert weights_generation() == gen + 2
    assert _same(_cpu(params), p0) and _same(_cpu(opt.ema_parameters()), e0)
    assert ptrs == [p.data_ptr() for p in params]


def test_state_dict_round_trips_the_ema():
    """state_dict() after three steps -> a fresh FusedAdamW on cloned parameters, load_state_dict + set_ema: one more step with the
    same gradients gives bit-equal p, m, v and ema.  A loaded state without "ema" seeds the average from the parameters."""
    params = _params(11)
    opt = _two_groups(params)
    opt.set_ema(0.99, warmup=True)
    g = torch.Generator().manual_seed(12)
    for step in range(3):
        grads = _grads(g)
        if step == 0:
            grads[2] = None
        _set_grads(params, grads)
        opt.step()
    sd = copy.deepcopy(opt.state_dict())
    assert all("ema" in st for st in sd["state"].values())
    twin = _params(11)
    for q, p in zip(twin, params):
        q.data.copy_(p.detach())
    topt = _two_groups(twin)
    topt.load_state_dict(sd)
    topt.set_ema(0.99, warmup=True)
    assert _same(_cpu(topt.ema_parameters()), _cpu(opt.ema_parameters()))
    assert not _same(_cpu(topt.ema_parameters()), _cpu(twin))
    last = _grads(g)
    for ps, o in ((params, opt), (twin, topt)):
        _set_grads(ps, last)
        o.step()
    assert _same(_cpu(params), _cpu(twin)) and _same(_cpu(opt.ema_parameters()), _cpu(topt.ema_parameters()))
    for i, ((sa, ma, va), (sb, mb, vb)) in enumerate(zip(_state(opt, params), _state(topt, twin))):
        assert sa == sb == (3.0 if i == 2 else 4.0) and torch.equal(ma, mb) and torch.equal(va, vb)
    # a state without "ema" (an optimizer that ran with the EMA off)
    bare = copy.deepcopy(sd)
    for st in bare["state"].values():
        del st["ema"]
    third = _params(11)
    oopt = _two_groups(third)
    oopt.load_state_dict(bare)
    oopt.set_ema(0.99)
    assert _same(_cpu(oopt.ema_parameters()), _cpu(third))


def test_set_ema_rejects_bad_arguments_and_the_entries_refuse_them():
    from dpft_amd.hip.lib import lib
    from dpft_amd.training.optimizer import FusedAdamW
    params = _params(13)[:1]
    opt = FusedAdamW(params, **HYPER)
    for bad in (1.0, 1, -0.1, 0.99999999, 10 ** 400, float("nan"), float("inf"), "0.9", True):
        with pytest.raises(ValueError):
            opt.set_ema(bad)
    with pytest.raises(ValueError):
        opt.set_ema(0.9, warmup=2)
    opt.set_ema(0.9)
    opt.set_ema(None)
    assert opt._ema is None
    one = C.c_void_p(256)                                                   # never dereferenced: refused before any launch

    def adamw_ema(decay=0.9, warmup=0, m_base=one, ema_base=one, chunks=one, n=1, step=1):
        return lib.dpft_adamw_ema_f32(chunks, n, None, None, 1e-3, 0.9, 0.999, 1e-8, 1e-2, step, None, None, m_base, ema_base,
                                      decay, warmup, None)
    for kw in (dict(decay=1.0), dict(decay=-0.1), dict(decay=float("nan")), dict(warmup=2), dict(ema_base=None),
               dict(m_base=None), dict(chunks=None), dict(n=0), dict(step=0)):
        assert adamw_ema(**kw) != 0, kw
        assert b"adamw_ema" in lib.dpft_last_error(), kw
    for rows, n in ((one, 0), (None, 1), (one, -1)):
        assert lib.dpft_swap_f32(rows, n, None) != 0
        assert b"swap" in lib.dpft_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# the trainer (the small configuration of tests/test_gpu_grad_clip.py: ResNet50 camera, batch 2, graphs enabled)
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = {"camera_mono": (96, 160, 3), "radar_bev": (128, 43, 6), "radar_front": (37, 107, 6)}
OPT_ENTRIES = {"dpft_adamw_f32", "dpft_adamw_clip_f32", "dpft_adamw_ema_f32", "dpft_swap_f32", "dpft_grad_sqnorm_f32",
               "dpft_grad_clip_coef_f32"}


def _trainer(ema, clip=None):
    from dpft_amd.configs import load_config
    from dpft_amd.models import build
    from dpft_amd.synthetic import make_batch, make_labels
    from dpft_amd.training.trainer import DataParallelTrainer
    cfg = copy.deepcopy(load_config("kradar"))
    cfg["model"]["backbones"]["camera_mono"]["name"] = "ResNet50"
    cfg["model"]["fuser"]["dropout"] = 0.0
    if ema is not None:
        cfg["train"]["ema"] = ema
    if clip is not None:
        cfg["train"]["clip_grad_norm"] = clip
    batch = make_batch(cfg["model"]["inputs"], 2, seed=9, shapes=SHAPES, device=DEV)
    labels = make_labels(2, seed=9, device=DEV)
    torch.manual_seed(0)
    tr = DataParallelTrainer(build("dprt", cfg), cfg, torch.device(DEV))
    tr.enable_graphs(batch)
    return tr, batch, labels


def _entry_names(monkeypatch, fn):
    """Names of the optimizer's C entries that pass through lib.call while fn() runs."""
    from dpft_amd.hip.lib import lib
    names, orig = [], lib.call

    def recording(name, *args):
        names.append(name)
        return orig(name, *args)
    with monkeypatch.context() as m:
        m.setattr(lib, "call", recording)
        fn()
    return [n for n in names if n in OPT_ENTRIES]


def test_trainer_without_the_key_launches_neither_new_entry(monkeypatch):
    tr, batch, labels = _trainer(None)
    assert tr.ema is None and tr.optimizer._ema is None and tr.ema_parameters() is None
    tr.train_step(batch, labels)
    called = _entry_names(monkeypatch, lambda: tr.train_step(batch, labels))
    assert called == ["dpft_adamw_f32"]
    with tr.ema_weights():                                                  # a no-op: no launch either
        pass
    assert all("ema" not in t and "swap" not in t for t in tr.optimizer._tables)
    assert all("ema" not in st for st in tr.optimizer.state.values())


def test_trainer_with_clipping_runs_the_norm_entries_then_the_ema_entry(monkeypatch):
    tr, batch, labels = _trainer(0.99, clip=0.1)
    tr.train_step(batch, labels)
    called = _entry_names(monkeypatch, lambda: tr.train_step(batch, labels))
    assert called == ["dpft_grad_sqnorm_f32", "dpft_grad_clip_coef_f32", "dpft_adamw_ema_f32"]
    assert float(tr.last_grad_norm) > 0.1


@pytest.fixture(scope="module")
def ema_trainer():
    """One trainer with "ema": 0.99 after three steps, shared by the tests below (each leaves weights and EMA as it found them)."""
    tr, batch, labels = _trainer(0.99)
    for _ in range(3):
        tr.train_step(batch, labels)
    torch.cuda.synchronize()
    return tr, batch, labels


@pytest.fixture(scope="module")
def ema_trainer_flags_off():
    """The same trainer built from {"decay": 0.99, "validate": false, "save": false}, after the same three steps."""
    tr, batch, labels = _trainer({"decay": 0.99, "validate": False, "save": False})
    for _ in range(3):
        tr.train_step(batch, labels)
    torch.cuda.synchronize()
    return tr, batch, labels


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def test_trainer_launches_the_ema_entry_once_per_step(ema_trainer, monkeypatch):
    from dpft_amd.training.optimizer import FusedAdamW
    tr, batch, labels = ema_trainer
    assert isinstance(tr.optimizer, FusedAdamW) and tr.ema == {"decay": 0.99, "warmup": False, "validate": True, "save": True}
    called = _entry_names(monkeypatch, lambda: tr.train_step(batch, labels))
    assert called == ["dpft_adamw_ema_f32"]
    live = [p for p in tr.model.parameters() if p.requires_grad]
    ema = tr.ema_parameters()
    assert len(ema) == len(live) and all(e.shape == p.shape for e, p in zip(ema, live))
    moved = torch.stack([(e != p.detach()).any() for e, p in zip(ema, live)]).cpu()
    assert int(moved.sum()) > 200


def test_eval_forward_under_the_ema_equals_a_twin_with_the_ema_as_weights(ema_trainer):
    """The eval-mode forward under ema_weights() against a deep copy of the model (taken outside the context) whose parameters
    were overwritten with ema_parameters(): a weight-derived cache that survived the swap (packed decoder blobs, split planes,
    bf16 copies) would show here.  torch.equal when the live model's eval forward is bit-reproducible run to run, the project's
    1e-4 relative rule for forward outputs otherwise.  After the context, parameters and EMA are bit-equal to before it."""
    from dpft_amd.hip.lib import note_weights_changed
    tr, batch, labels = ema_trainer
    live = [p for p in tr.model.parameters() if p.requires_grad]
    p0, e0 = _cpu(live), _cpu(tr.ema_parameters())
    tr.model.eval()
    with torch.no_grad():
        first = {k: v.clone() for k, v in tr.model(batch).items()}
        second = {k: v.clone() for k, v in tr.model(batch).items()}
        reproducible = all(torch.equal(first[k], second[k]) for k in first)
        print(f"eval forward bit-reproducible run to run: {reproducible}")
        twin = copy.deepcopy(tr.model)
        for q, e in zip([q for q in twin.parameters() if q.requires_grad], tr.ema_parameters()):
            q.data.copy_(e)
        note_weights_changed()
        twin.eval()
        want = {k: v.clone() for k, v in twin(batch).items()}
        with tr.ema_weights():
            got = {k: v.clone() for k, v in tr.model(batch).items()}
        after = {k: v.clone() for k, v in tr.model(batch).items()}
    for k in want:
        print(f"{k}: rel(ema forward, twin) = {_rel(got[k], want[k]):.3e}; rel(ema forward, live forward) = {_rel(got[k], first[k]):.3e}")
        if reproducible:
            assert torch.equal(got[k], want[k]), k
            assert torch.equal(after[k], first[k]), k
        else:
            assert _rel(got[k], want[k]) < 1e-4, k
            assert _rel(after[k], first[k]) < 1e-4, k
    assert any(not torch.equal(got[k], first[k]) for k in got), "the EMA forward must differ from the live one"
    assert _same(_cpu(live), p0) and _same(_cpu(tr.ema_parameters()), e0)


def test_validation_runs_under_the_ema_unless_switched_off(ema_trainer, ema_trainer_flags_off):
    """validate_one_epoch on a one-batch loader returns the loss computed by hand under ema_weights(); a trainer built with
    "validate": false in its config returns the live-weight loss."""
    tr, batch, labels = ema_trainer
    live = [p for p in tr.model.parameters() if p.requires_grad]
    p0, e0 = _cpu(live), _cpu(tr.ema_parameters())
    tr.model.eval()
    tr.loss_fn.eval()
    with torch.no_grad():
        live_loss = float(tr.loss_fn(tr.model(batch), labels)[0])
        reproducible = float(tr.loss_fn(tr.model(batch), labels)[0]) == live_loss
        with tr.ema_weights():
            ema_loss = float(tr.loss_fn(tr.model(batch), labels)[0])
    got = tr.validate_one_epoch(0, [(batch, labels)])["loss"]
    off, _, _ = ema_trainer_flags_off                  # built with "validate": false: its own weights, its own two losses
    assert off.ema["validate"] is False
    off.model.eval()
    off.loss_fn.eval()
    with torch.no_grad():
        off_live = float(off.loss_fn(off.model(batch), labels)[0])
        with off.ema_weights():
            off_ema = float(off.loss_fn(off.model(batch), labels)[0])
    got_live = off.validate_one_epoch(0, [(batch, labels)])["loss"]
    print(f"live loss {live_loss!r}, ema loss {ema_loss!r}, validate {got!r}; built with validate false: live {off_live!r}, "
          f"ema {off_ema!r}, validate {got_live!r}; reproducible {reproducible}")
    assert ema_loss != live_loss and off_ema != off_live
    if reproducible:                                # the same launches on the same bits: the same loss
        assert got == ema_loss and got_live == off_live
    else:                                           # (the 1e-4 relative rule of forward outputs, far below what tells the two apart)
        assert abs(ema_loss - live_loss) > 1e-3 * abs(live_loss) and abs(off_ema - off_live) > 1e-3 * abs(off_live)
        assert abs(got - ema_loss) <= 1e-4 * abs(ema_loss) and abs(got_live - off_live) <= 1e-4 * abs(off_live)
    assert _same(_cpu(live), p0) and _same(_cpu(tr.ema_parameters()), e0)


def test_checkpoint_writes_the_ema_module_next_to_the_plain_one(ema_trainer, ema_trainer_flags_off, tmp_path):
    from dpft_amd.models import load
    tr, batch, labels = ema_trainer
    live = [p for p in tr.model.parameters() if p.requires_grad]
    p0, e0 = _cpu(live), _cpu(tr.ema_parameters())
    tr.save_checkpoint(str(tmp_path / "t_checkpoint_0002.pt"))
    assert sorted(os.listdir(tmp_path)) == ["t_checkpoint_0002.pt", "t_checkpoint_0002_ema.pt"]
    plain, epoch, _ = load(str(tmp_path / "t_checkpoint_0002.pt"))
    shipped, epoch_e, _ = load(str(tmp_path / "t_checkpoint_0002_ema.pt"))
    assert epoch == epoch_e == 2
    assert _same(_cpu([q for q in plain.parameters() if q.requires_grad]), p0)
    assert _same(_cpu([q for q in shipped.parameters() if q.requires_grad]), e0)
    assert _same(_cpu(live), p0) and _same(_cpu(tr.ema_parameters()), e0)
    off, _, _ = ema_trainer_flags_off                  # built with "save": false in its config
    assert off.ema["save"] is False
    off.save_checkpoint(str(tmp_path / "u_checkpoint_0002.pt"))
    assert sorted(os.listdir(tmp_path)) == ["t_checkpoint_0002.pt", "t_checkpoint_0002_ema.pt", "u_checkpoint_0002.pt"]
