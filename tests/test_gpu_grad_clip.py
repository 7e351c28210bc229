"""Gradient clipping by global L2 norm on the device: dpft_grad_sqnorm_f32, dpft_grad_clip_coef_f32 and dpft_adamw_clip_f32
through FusedAdamW.set_clip and the trainer's ``train.clip_grad_norm`` key, against the fp64 reference of tests/grad_clip_ref.py
(vetted against torch in tests/test_grad_clip_host.py) and against torch itself.

The tensors are those of the AdamW edge test: ends on a CHUNK = 16384 boundary, one short of it and one past it, two chunks + 7,
moment offsets of every residue mod 4, and one parameter that is a view at storage offset 1 (4-byte aligned only)."""
import copy

import numpy as np
import pytest
import torch

from tests import grad_clip_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
ADAM_NUMELS = [3, 16384, 5, 16385, 1, 16383, 4, 32775]      # moment offsets 0, 3, 16387, 16392, 32777, 32778, 49161, 49165
HYPER = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)


def _params(seed, numels=ADAM_NUMELS):
    """(parameters on the device, their initial values on the CPU); numel 16385 is a view at storage offset 1."""
    g = torch.Generator().manual_seed(seed)
    params, p0 = [], []
    for n in numels:
        init = torch.randn(n, generator=g)
        if n == 16385:
            store = torch.empty(n + 1, device=DEV)
            p = torch.nn.Parameter(store[1:])
            assert p.data_ptr() % 16 == 4
        else:
            p = torch.nn.Parameter(torch.empty(n, device=DEV))
            assert p.data_ptr() % 16 == 0
        p.data.copy_(init)
        params.append(p)
        p0.append(init)
    return params, p0


def _grads(g, numels=ADAM_NUMELS, scale=1.0):
    """Random gradients (CPU, fp32) with exact zeros: a tenth of the elements and every tensor's last element."""
    out = []
    for n in numels:
        gr = torch.randn(n, generator=g) * scale
        gr[torch.rand(n, generator=g) < 0.1] = 0.0
        if n >= 4:
            gr[n - 1] = 0.0
        out.append(gr)
    return out


def _set_grads(params, grads):
    for p, gr in zip(params, grads):
        p.grad = None if gr is None else gr.to(DEV)


def _record(opt):
    """The clip record as (norm, coef, nonfinite, nonfinite_total) + its raw words."""
    torch.cuda.synchronize()
    words = opt._clip_record.cpu()
    f = words.view(torch.float32)
    return np.float32(f[0].item()), np.float32(f[1].item()), int(words[2]), int(words[3]), words


def _np(grads):
    return [None if gr is None else gr.numpy() for gr in grads]


def _state(opt, params):
    sd = opt.state_dict()["state"]
    return [(float(sd[i]["step"]), sd[i]["exp_avg"].detach().cpu().clone(), sd[i]["exp_avg_sq"].detach().cpu().clone())
            for i in range(len(params))]


def test_norm_and_coefficient_against_fp64_and_bit_reproducible():
    """Two parameter groups (two chunk tables, disjoint ranges of one partials buffer), one tensor without a gradient, exact zeros
    among the gradients.  norm within 1 fp32 ulp of the fp64 value (an fp64 sum of < 1e8 exact squares is good to ~1e-8
    relative, far inside an ulp: only the final rounding shows), coef within 2 ulp; the per-tensor squared norms of
    grad_sqnorms() are the fp64 ones (1e-12 relative: they only differ in summation order); the two norm launches run twice on
    the same gradients give bit-equal partials and a bit-equal record."""
    from dpft_amd.training.optimizer import FusedAdamW
    params, _ = _params(1)
    opt = FusedAdamW([{"params": params[:4]}, {"params": params[4:], "lr": 3e-3}], **HYPER)
    max_norm = 0.5
    opt.set_clip(max_norm)
    assert opt.last_grad_norm() is not None and float(opt.last_grad_norm()) == 0.0 and opt.nonfinite_steps() == 0
    grads = _grads(torch.Generator().manual_seed(2))
    grads[2] = None                                                        # numel 5: grad is None
    _set_grads(params, grads)
    opt.step()
    norm, coef, nonfinite, total, words = _record(opt)
    want_norm, want_coef = R.norm_coef(_np(grads), R.f32(max_norm))
    print(f"norm {norm!r} vs {want_norm!r}: {R.ulps_f32(norm, want_norm):.3f} ulp; coef {coef!r} vs {want_coef!r}: "
          f"{R.ulps_f32(coef, want_coef):.3f} ulp")
    assert want_coef < 1.0 and (nonfinite, total) == (0, 0)
    assert R.ulps_f32(norm, want_norm) <= 1.0
    assert R.ulps_f32(coef, want_coef) <= 2.0
    assert float(opt.last_grad_norm()) == float(norm) and opt.last_grad_norm().is_cuda
    # per-tensor squared norms, on demand
    per = torch.cat(opt.grad_sqnorms()).cpu().numpy()
    want = np.array([0.0 if gr is None else R.sqnorm([gr]) for gr in _np(grads)])
    assert per.shape == (len(ADAM_NUMELS),) and per[2] == 0.0
    np.testing.assert_allclose(per, want, rtol=1e-12, atol=0)
    rows = len(ADAM_NUMELS) + sum(-(-n // 16384) for n, gr in zip(ADAM_NUMELS, grads) if gr is not None)      # markers + chunks
    assert opt._partials.numel() == sum(t["n_chunks"] for t in opt._tables) == rows == 18
    # the two launches again, twice, on the same gradients: the same bits
    runs = []
    for _ in range(2):
        opt._partials.fill_(float("nan"))
        opt._launch_norm()
        torch.cuda.synchronize()
        runs.append((opt._partials.cpu().view(torch.int64).clone(), opt._clip_record.cpu().clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][1], words)


@pytest.mark.parametrize("value", [3e19, 1e-30])
def test_norm_survives_squares_outside_the_fp32_range(value):
    """Every element 3e19 (the squares overflow fp32) or 1e-30 (the squares flush to zero in fp32): the elements are widened to
    double before they are squared, so the norm is finite and correct to 1 ulp."""
    from dpft_amd.training.optimizer import FusedAdamW
    params, _ = _params(3)
    opt = FusedAdamW(params, **HYPER)
    opt.set_clip(0.1)
    grads = [torch.full((n,), value, dtype=torch.float32) for n in ADAM_NUMELS]
    sq = np.float32(value) * np.float32(value)
    assert not np.isfinite(sq) or sq == 0.0                                # fp32 squares would be useless
    _set_grads(params, grads)
    opt.step()
    norm, coef, nonfinite, total, _ = _record(opt)
    want_norm, want_coef = R.norm_coef(_np(grads), R.f32(0.1))
    print(f"value {value}: norm {norm!r} vs {want_norm!r}: {R.ulps_f32(norm, want_norm):.3f} ulp")
    assert np.isfinite(norm) and norm > 0 and (nonfinite, total) == (0, 0)
    assert R.ulps_f32(norm, want_norm) <= 1.0
    assert R.ulps_f32(coef, want_coef) <= 2.0


def test_coefficient_one_is_the_unclipped_step_bit_for_bit():
    """max_norm = 1e30: coef == 1.0f, and three steps give parameters, moments and step counts bit-equal to a twin optimizer
    without clipping (g * 1.0f == g)."""
    from dpft_amd.training.optimizer import FusedAdamW
    pa, _ = _params(4)
    pb, _ = _params(4)
    oa, ob = FusedAdamW(pa, **HYPER), FusedAdamW(pb, **HYPER)
    ob.set_clip(1e30)
    g = torch.Generator().manual_seed(5)
    for _ in range(3):
        grads = _grads(g)
        _set_grads(pa, grads)
        _set_grads(pb, grads)
        oa.step()
        ob.step()
        assert _record(ob)[1] == np.float32(1.0)
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach(), b.detach())
    for (sa, ma, va), (sb, mb, vb) in zip(_state(oa, pa), _state(ob, pb)):
        assert sa == sb == 3.0 and torch.equal(ma, mb) and torch.equal(va, vb)


MAX_NORM = 1.0      # the gradients of _grads() over 98 310 elements have a norm of ~300: the coefficient is ~0.003 in every step


@pytest.fixture(scope="module")
def clipped_run():
    """Three clipped steps of FusedAdamW on the edge tensors, run once: the gradients, the initial values and the results."""
    from dpft_amd.training.optimizer import CHUNK, FusedAdamW
    assert CHUNK == 16384
    params, p0 = _params(6)
    opt = FusedAdamW(params, **HYPER)
    opt.set_clip(MAX_NORM)
    g = torch.Generator().manual_seed(7)
    steps, records = [], []
    for _ in range(3):
        grads = _grads(g)
        _set_grads(params, grads)
        assert all(p.grad.data_ptr() % 16 == 0 for p in params)
        opt.step()
        records.append(_record(opt)[:2])
        assert all(torch.equal(p.grad.cpu(), gr) for p, gr in zip(params, grads)), ".grad must keep the unclipped gradient"
        steps.append(grads)
    torch.cuda.synchronize()
    return dict(p0=p0, steps=steps, records=records, p=[p.detach().cpu().clone() for p in params], state=_state(opt, params))


def test_clipped_update_against_the_fp64_recurrence(clipped_run):
    """p, m and v after three clipped steps, element by element, against the fp64 recurrence with g * coef, inside the running
    first-order bound of tests/grad_clip_ref.py: the 14 roundings of adamw_kernel per element and step plus
    E_g = 3 u |g coef| for the clipped gradient (one rounding of the product + the coefficient's distance from the fp64 one),
    carried into E_m through c1 and into E_v through 2 c2 |g'|.  The coefficient is below 1 in every step (asserted in the
    reference), and the derived bound on p lies inside the rtol 1e-5 + 1e-6 max|p| of the comparison with torch."""
    ref = R.AdamWRef([t.numpy() for t in clipped_run["p0"]], kernel_scalars=True, **HYPER)
    for grads, (norm, coef) in zip(clipped_run["steps"], clipped_run["records"]):
        want_norm, want_coef = ref.clipped_step(_np(grads), MAX_NORM)
        assert want_coef < 0.01
        assert R.ulps_f32(norm, want_norm) <= 1.0 and R.ulps_f32(coef, want_coef) <= 2.0
    offs = np.cumsum([0] + ADAM_NUMELS[:-1])
    for i, n in enumerate(ADAM_NUMELS):
        step, m, v = clipped_run["state"][i]
        assert step == 3.0
        pmax = float(np.abs(ref.P[i]).max())
        assert (ref.EP[i] < 1e-5 * np.abs(ref.P[i]) + 1e-6 * pmax).all(), f"numel {n}: the derived bound is not tighter than the torch comparison"
        for name, got, want, err in (("p", clipped_run["p"][i], ref.P[i], ref.EP[i]), ("m", m, ref.M[i], ref.EM[i]),
                                     ("v", v, ref.V[i], ref.EV[i])):
            got = got.double().numpy().reshape(-1)
            diff = np.abs(got - want)
            w = int(np.argmax(diff - err))
            print(f"clipped adamw numel {n} {name}: max |diff| / bound = {float((diff / np.maximum(err, 1e-300)).max()):.3f}")
            assert (diff <= err).all(), (f"numel {n} (moment offset {int(offs[i])}), {name}: {int((diff > err).sum())} elements above "
                                         f"the bound; worst at {w}: |{got[w]!r} - {want[w]!r}| = {diff[w]:.3e} > {err[w]:.3e}")


def _close(a, b, what, rtol=1e-5, atol_scale=1e-6):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    atol = atol_scale * max(float(b.abs().max()), 1e-6)
    torch.testing.assert_close(a, b, rtol=rtol, atol=atol, msg=lambda m: f"{what}: {m}")


def test_clipped_update_against_torch(clipped_run):
    """The same three steps with torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW on fp32 clones, at the project's tolerance for
    that comparison (rtol 1e-5, atol 1e-6 max|p|)."""
    ref = [torch.nn.Parameter(t.clone().to(DEV)) for t in clipped_run["p0"]]
    opt = torch.optim.AdamW(ref, **HYPER)
    for grads, (norm, _) in zip(clipped_run["steps"], clipped_run["records"]):
        _set_grads(ref, grads)
        want = torch.nn.utils.clip_grad_norm_(ref, MAX_NORM)
        opt.step()
        assert abs(float(norm) - float(want)) <= 1e-5 * float(want)
    for i, (r, n) in enumerate(zip(ref, ADAM_NUMELS)):
        _close(clipped_run["p"][i], r, f"numel {n} p")
        _close(clipped_run["state"][i][1], opt.state[r]["exp_avg"], f"numel {n} exp_avg")
        _close(clipped_run["state"][i][2], opt.state[r]["exp_avg_sq"], f"numel {n} exp_avg_sq")


def test_closed_gate_with_clipping_updates_nothing():
    """gate = 0 with clipping on: no parameter or moment moves and every tensor's `skipped` advances (its own step count stays)."""
    from dpft_amd.training.optimizer import FusedAdamW
    params, _ = _params(8)
    opt = FusedAdamW(params, **HYPER)
    opt.set_clip(MAX_NORM)
    g = torch.Generator().manual_seed(9)
    _set_grads(params, _grads(g))
    opt.step()
    before, state = [p.detach().clone() for p in params], _state(opt, params)
    skipped = opt._tables[0]["skipped"].cpu().clone()
    _set_grads(params, _grads(g))
    opt.set_gate(torch.tensor(0.0, device=DEV))
    opt.step()
    torch.cuda.synchronize()
    assert all(torch.equal(p.detach(), b) for p, b in zip(params, before))
    assert torch.equal(opt._tables[0]["skipped"].cpu(), skipped + 1)
    for (s0, m0, v0), (s1, m1, v1) in zip(state, _state(opt, params)):
        assert s0 == s1 == 1.0 and torch.equal(m0, m1) and torch.equal(v0, v1)


def test_nan_gradient_propagates_like_torch():
    """"propagate" (the default): a NaN in one gradient makes the norm and the coefficient NaN and with them every parameter that
    has a gradient, exactly where torch's clip_grad_norm_ + AdamW (the twin, on the CPU) makes them NaN; nonfinite is flagged,
    nothing is counted as skipped."""
    from dpft_amd.training.optimizer import FusedAdamW
    params, p0 = _params(10)
    opt = FusedAdamW(params, **HYPER)
    opt.set_clip(MAX_NORM)
    twin = [torch.nn.Parameter(t.clone()) for t in p0]
    topt = torch.optim.AdamW(twin, **HYPER)
    grads = _grads(torch.Generator().manual_seed(11))
    grads[3][100] = float("nan")
    grads[4] = None                                                        # a tensor without a gradient stays finite
    _set_grads(params, grads)
    for q, gr in zip(twin, grads):
        q.grad = None if gr is None else gr.clone()
    torch.nn.utils.clip_grad_norm_([q for q in twin if q.grad is not None], MAX_NORM)
    topt.step()
    opt.step()
    norm, coef, nonfinite, total, _ = _record(opt)
    assert np.isnan(norm) and np.isnan(coef) and (nonfinite, total) == (1, 0) and opt.nonfinite_steps() == 0
    for i, (p, q) in enumerate(zip(params, twin)):
        assert torch.equal(torch.isnan(p.detach().cpu()), torch.isnan(q.detach())), i
        assert bool(torch.isnan(p.detach()).all()) == (grads[i] is not None)
    assert torch.equal(params[4].detach().cpu(), p0[4])


def test_nan_gradient_in_skip_mode_drops_the_step():
    """"skip": the step with a NaN gradient leaves parameters and moments bit-equal to before and is counted
    (nonfinite_steps() == 1); the next clean step equals the twin that never saw the bad step, the per-parameter step counts of
    state_dict() included."""
    from dpft_amd.training.optimizer import FusedAdamW
    pa, _ = _params(12)
    pb, _ = _params(12)
    oa, ob = FusedAdamW(pa, **HYPER), FusedAdamW(pb, **HYPER)
    oa.set_clip(MAX_NORM, nonfinite="skip")
    ob.set_clip(MAX_NORM, nonfinite="skip")
    g = torch.Generator().manual_seed(13)
    first, bad, clean = _grads(g), _grads(g), _grads(g)
    bad[7][20000] = float("nan")
    for ps, o in ((pa, oa), (pb, ob)):
        _set_grads(ps, first)
        o.step()
    before, state = [p.detach().clone() for p in pa], _state(oa, pa)
    _set_grads(pa, bad)
    oa.step()                                                              # only `a` sees the bad step
    norm, coef, nonfinite, total, _ = _record(oa)
    assert np.isnan(norm) and (nonfinite, total) == (1, 1) and oa.nonfinite_steps() == 1
    assert all(torch.equal(p.detach(), b) for p, b in zip(pa, before))
    for (s0, m0, v0), (s1, m1, v1) in zip(state, _state(oa, pa)):
        assert s0 == s1 == 1.0 and torch.equal(m0, m1) and torch.equal(v0, v1)
    for ps, o in ((pa, oa), (pb, ob)):
        _set_grads(ps, clean)
        o.step()
    assert _record(oa)[2:4] == (0, 1) and ob.nonfinite_steps() == 0          # the flag is per step, the counter stays
    assert _record(oa)[:2] == _record(ob)[:2]
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach(), b.detach())
    for (sa, ma, va), (sb, mb, vb) in zip(_state(oa, pa), _state(ob, pb)):
        assert sa == sb == 2.0 and torch.equal(ma, mb) and torch.equal(va, vb)


def test_set_clip_rejects_bad_arguments_and_the_entries_refuse_them():
    import ctypes as C
    from dpft_amd.hip.lib import lib
    from dpft_amd.training.optimizer import FusedAdamW
    params, _ = _params(14, numels=[5])
    opt = FusedAdamW(params, **HYPER)
    for bad in (0.0, -1.0, float("inf"), float("nan"), "1", True):
        with pytest.raises(ValueError):
            opt.set_clip(bad)
    with pytest.raises(ValueError):
        opt.set_clip(1.0, nonfinite="ignore")
    opt.set_clip(1.0)
    opt.set_clip(None)
    assert opt._clip is None
    one = C.c_void_p(256)                                                   # never dereferenced: refused before any launch
    for max_norm, mode in ((0.0, 0), (-1.0, 0), (float("inf"), 0), (float("nan"), 0), (1.0, 2), (1.0, -1)):
        assert lib.dpft_grad_clip_coef_f32(one, 1, max_norm, mode, one, None) == -1
        assert b"grad_clip_coef:" in lib.dpft_last_error()


def test_segments_are_left_to_step_while_clipping_is_on():
    """With segments attached and clipping on step_segment() returns False (no bucket can be stepped before the norm of all
    buckets is known) and step() does everything: the same bits as the clipped optimizer without segments."""
    from dpft_amd.training.optimizer import FusedAdamW
    pa, _ = _params(15)
    pb, _ = _params(15)
    oa, ob = FusedAdamW(pa, **HYPER), FusedAdamW(pb, **HYPER)
    ob.attach_segments([pb[0:3], pb[3:5], pb[5:7]])                         # pb[7] belongs to no segment
    oa.set_clip(MAX_NORM)
    ob.set_clip(MAX_NORM)
    g = torch.Generator().manual_seed(16)
    for step in range(3):
        grads = _grads(g)
        for ps in (pa, pb):
            for p, gr in zip(ps, grads):
                p.grad = gr.to(DEV) if p.grad is None else p.grad.copy_(gr.to(DEV))      # persistent gradient buffers
        oa.step()
        assert [ob.step_segment(si) for si in (2, 0, 1)] == [False, False, False]
        ob.step()
        assert _record(oa)[:2] == _record(ob)[:2] and _record(ob)[1] < 1
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach(), b.detach())
    for (sa, ma, va), (sb, mb, vb) in zip(_state(oa, pa), _state(ob, pb)):
        assert sa == sb == 3.0 and torch.equal(ma, mb) and torch.equal(va, vb)
    ob.set_clip(None)                                                       # clipping off again: segments step early as before
    for p, gr in zip(pb, _grads(g)):
        p.grad.copy_(gr.to(DEV))
    assert all(ob.step_segment(si) for si in (2, 0, 1))
    ob.step()


# ---------------------------------------------------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = {"camera_mono": (96, 160, 3), "radar_bev": (128, 43, 6), "radar_front": (37, 107, 6)}
NEW_ENTRIES = {"dpft_grad_sqnorm_f32", "dpft_grad_clip_coef_f32", "dpft_adamw_clip_f32"}


def _trainer(clip, monkeypatch=None):
    from dpft_amd.configs import load_config
    from dpft_amd.models import build
    from dpft_amd.synthetic import make_batch, make_labels
    from dpft_amd.training.trainer import DataParallelTrainer
    cfg = copy.deepcopy(load_config("kradar"))
    cfg["model"]["backbones"]["camera_mono"]["name"] = "ResNet50"
    cfg["model"]["fuser"]["dropout"] = 0.0
    if clip is not None:
        cfg["train"]["clip_grad_norm"] = clip
    batch = make_batch(cfg["model"]["inputs"], 2, seed=9, shapes=SHAPES, device=DEV)
    labels = make_labels(2, seed=9, device=DEV)
    torch.manual_seed(0)
    tr = DataParallelTrainer(build("dprt", cfg), cfg, torch.device(DEV))
    tr.enable_graphs(batch)
    return tr, batch, labels


def _entry_names(monkeypatch, fn):
    """Names of the C entries that pass through lib.call while fn() runs."""
    from dpft_amd.hip.lib import lib
    names, orig = [], lib.call

    def recording(name, *args):
        names.append(name)
        return orig(name, *args)
    with monkeypatch.context() as m:
        m.setattr(lib, "call", recording)
        fn()
    return names


def test_trainer_clips_on_the_device_and_matches_clipped_torch_adamw(monkeypatch):
    """train.clip_grad_norm = 0.1 on the small training config (ResNet50 camera, batch 2, graphs enabled; early AdamW stays off
    even with DPFT_EARLY_ADAMW=1).  One train_step from a snapshot of parameters and optimizer state: the unclipped gradients
    are still in .grad afterwards; their fp64 norm is trainer.last_grad_norm to 1 ulp; clip_grad_norm_ + torch.optim.AdamW
    applied to the snapshot with those gradients gives the trainer's parameters at rtol 1e-5 + 1e-6 max|p|."""
    from dpft_amd.training.optimizer import FusedAdamW
    monkeypatch.setenv("DPFT_EARLY_ADAMW", "1")
    tr, batch, labels = _trainer(0.1)
    assert isinstance(tr.optimizer, FusedAdamW) and tr.clip == (0.1, "propagate") and not tr.early_adamw
    assert tr.reducer.on_bucket_final is None and float(tr.last_grad_norm) == 0.0
    tr.train_step(batch, labels)                                            # builds the tables and the moments
    names = [n for n, _ in tr.model.named_parameters()]
    plist = list(tr.model.parameters())
    snap = [p.detach().clone() for p in plist]
    sd = copy.deepcopy(tr.optimizer.state_dict())
    called = _entry_names(monkeypatch, lambda: tr.train_step(batch, labels))
    assert called.count("dpft_grad_sqnorm_f32") == 1 and called.count("dpft_grad_clip_coef_f32") == 1
    assert called.count("dpft_adamw_clip_f32") == 1 and "dpft_adamw_f32" not in called
    assert called.index("dpft_grad_sqnorm_f32") < called.index("dpft_grad_clip_coef_f32") < called.index("dpft_adamw_clip_f32")
    torch.cuda.synchronize()
    seen = tr.reducer.seen_ids()
    grads = [p.grad.detach().clone() if (p.grad is not None and id(p) in seen) else None for p in plist]
    assert sum(g is not None for g in grads) > 200
    want_norm = R.norm_coef([None if g is None else g.cpu().numpy() for g in grads], R.f32(0.1))[0]
    got_norm = np.float32(tr.last_grad_norm.item())
    print(f"trainer grad norm {got_norm!r} vs fp64 {want_norm!r}: {R.ulps_f32(got_norm, want_norm):.3f} ulp")
    assert tr.last_grad_norm.is_cuda and want_norm > 0.1, "the clip must bite for this test to mean anything"
    assert R.ulps_f32(got_norm, want_norm) <= 1.0
    # clipped torch AdamW from the snapshot, with the optimizer state in torch's own format
    twin = [torch.nn.Parameter(s.clone()) for s in snap]
    hyper = {k: tr.optimizer.param_groups[0][k] for k in ("lr", "betas", "eps", "weight_decay")}
    topt = torch.optim.AdamW(twin, **hyper)
    tsd = topt.state_dict()
    tsd["state"] = sd["state"]                                              # (the moments and per-parameter step counts only)
    topt.load_state_dict(tsd)
    for q, g in zip(twin, grads):
        q.grad = g
    torch.nn.utils.clip_grad_norm_([q for q in twin if q.grad is not None], 0.1)
    topt.step()
    ok, moved = [], []                                                      # compared on the device: one read-back for ~1 650 tensors
    for p, q, s in zip(plist, twin, snap):
        a, b = p.detach().double(), q.detach().double()
        atol = 1e-6 * torch.clamp(b.abs().max(), min=1e-6)
        ok.append(((a - b).abs() <= atol + 1e-5 * b.abs()).all())
        moved.append((p.detach() != s).any())
    ok, moved = torch.stack(ok).cpu(), torch.stack(moved).cpu()
    assert bool(ok.all()), [names[i] for i in torch.nonzero(~ok).flatten().tolist()][:10]
    assert int(moved.sum()) > 200 and len(names) == len(plist)


def test_trainer_without_the_key_launches_none_of_the_new_entries(monkeypatch):
    """Key absent: the step runs the launches it always ran -- none of the three new entries passes through lib.call, the
    optimizer is the one dpft_adamw_f32 launch, and the trainer reports no gradient norm."""
    tr, batch, labels = _trainer(None)
    assert tr.clip is None and tr.optimizer._clip is None and tr.optimizer._clip_record is None
    tr.train_step(batch, labels)
    called = _entry_names(monkeypatch, lambda: tr.train_step(batch, labels))
    assert not (NEW_ENTRIES & set(called)), sorted(NEW_ENTRIES & set(called))
    assert called.count("dpft_adamw_f32") == 1
    assert tr.last_grad_norm is None and tr.optimizer._partials is None
