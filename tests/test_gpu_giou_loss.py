"""The criterion's optional GIoU3D term on the device: dpft_giou_loss_fwd/bwd_f32 (dpft_amd/csrc/giou_loss.hip) against the
fp64 restatement of tests/giou_loss_ref.py, the two gradient forms, and the term inside ``Loss`` and the trainer.

Bound of the kernel checks: the kernel computes in fp64 and rounds once, 2^-24 relative; four times that is allowed for the
device's fp64 sin / cos / atan2 against the host's: |got - ref| <= 2^-22 * s, with s = |ref| (floor 2^-22 absolute) for
G / term / total and s = max|ref gradient| over the pair's eight components for a gradient."""
import copy
import ctypes as C

import pytest
import torch

from tests import giou_loss_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 2.0 ** -22


def _bound(ref):
    """|got - ref| <= 2^-22 * s with s = |ref|, floored at 2^-22: the stricter of the two readings of "floor 2^-22 absolute" (the
    floor is on the scale s, not on the bound)."""
    return TOL * max(abs(ref), TOL)
W = 2.0
TOTAL_IN = 1.25


def _tables():
    """The whole lattice in B = 3, N = 7, Mmax = 5 tables with matched counts (5, 0, 2) (the last one takes what is left),
    then the named classes again in N = 3 tables with five target rows: 3 pairs, the clamp min(N, m)."""
    out = []
    for n, k in enumerate(range(0, len(R.LATTICE), 7)):
        chunk = R.LATTICE[k:k + 7]
        out.append(R.pack([chunk[:5], [], chunk[5:]], N=7, Mmax=5, seed=n))
    valid = [p for p in R.NAMED if p["name"] not in R.INVALID]
    out.append(R.pack([valid[:3], valid[3:6]], N=3, Mmax=5, seed=100))
    out.append(R.pack([valid[6:8] + [R.NAMED[8]], [R.NAMED[9]] + R.LATTICE[10:12]], N=3, Mmax=5, seed=101))
    return out


@pytest.fixture(scope="module")
def tables():
    """[(table on the device, fp64 reference)], computed once and left unchanged."""
    got = []
    for t in _tables():
        ref = R.table_reference(t, W, TOTAL_IN)
        dev = {k: v.to(DEV) for k, v in t.items() if k != "where"}
        dev["where"] = t["where"]
        got.append((dev, ref))
    assert tuple(int(c) for c in got[0][0]["counts"]) == (5, 0, 2)
    assert sum(len(w) for t, _ in got[:-2] for w in t["where"]) == len(R.LATTICE)
    return got


def _sizes(t):
    return t["center"].shape[0], t["center"].shape[1], t["gt_box"].shape[1]


def _fwd(t, w=W, total_in=TOTAL_IN):
    from dpft_amd.hip.lib import lib, stream
    B, N, Mmax = _sizes(t)
    tin = torch.tensor(total_in, dtype=torch.float32, device=DEV)
    term, total = torch.empty((), device=DEV), torch.empty((), device=DEV)
    G = torch.full((B, Mmax), float("nan"), device=DEV)
    lib.call("dpft_giou_loss_fwd_f32", t["center"].data_ptr(), t["size"].data_ptr(), t["angle"].data_ptr(), t["gt_box"].data_ptr(),
             t["match"].data_ptr(), t["counts"].data_ptr(), w, tin.data_ptr(), term.data_ptr(), total.data_ptr(), G.data_ptr(),
             B, N, Mmax, stream())
    return term, total, G


def _bwd(t, w=W, gout=None, into=None):
    """Write form into fresh buffers, or the accumulate form into ``into``."""
    from dpft_amd.hip.lib import lib, stream
    B, N, Mmax = _sizes(t)
    bufs = into if into is not None else tuple(torch.full_like(t[k], float("nan")) for k in ("center", "size", "angle"))
    lib.call("dpft_giou_loss_bwd_f32", t["center"].data_ptr(), t["size"].data_ptr(), t["angle"].data_ptr(), t["gt_box"].data_ptr(),
             t["match"].data_ptr(), t["counts"].data_ptr(), w, None if gout is None else gout.data_ptr(), bufs[0].data_ptr(),
             bufs[1].data_ptr(), bufs[2].data_ptr(), 1 if into is not None else 0, B, N, Mmax, stream())
    return bufs


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return bool((_bits(a) == _bits(b)).all())


def _matched_rows(t):
    B, N, _ = _sizes(t)
    m = torch.zeros(B, N, dtype=torch.bool)
    for b, rows in enumerate(t["where"]):
        for i, _p in rows:
            m[b, i] = True
    return m


def test_kernel_against_fp64_on_the_lattice(tables):
    worst = {"G": 0.0, "term": 0.0, "total": 0.0, "grad": 0.0}
    for t, ref in tables:
        term, total, G = _fwd(t)
        grads = [g.double().cpu() for g in _bwd(t)]
        G = G.double().cpu()
        for name, got, want in (("term", float(term), ref["term"]), ("total", float(total), ref["total"])):
            err = abs(got - want)
            worst[name] = max(worst[name], err / max(abs(want), 1.0))
            assert err <= _bound(want), (name, got, want)
        rg = torch.cat((ref["dcenter"], ref["dsize"], ref["dangle"]), -1)            # (B,N,8)
        gg = torch.cat(grads, -1)
        matched = _matched_rows(t)
        assert not gg[~matched].any(), "rows of unmatched queries must be exactly 0"
        for b, rows in enumerate(t["where"]):
            for k, (i, p) in enumerate(rows):
                err = abs(float(G[b, k]) - float(ref["G"][b, k]))
                worst["G"] = max(worst["G"], err / max(abs(float(ref["G"][b, k])), 1.0))
                assert err <= _bound(float(ref["G"][b, k])), (p["name"], float(G[b, k]), float(ref["G"][b, k]))
                if p["name"] in R.INVALID:
                    assert float(G[b, k]) == -1.0 and not gg[b, i].any(), p["name"]
                    continue
                s = float(rg[b, i].abs().max())
                assert s > 0, p["name"]
                err = float((gg[b, i] - rg[b, i]).abs().max())
                worst["grad"] = max(worst["grad"], err / s)
                assert err <= TOL * s, (p["name"], gg[b, i].tolist(), rg[b, i].tolist())
            assert not G[b, len(rows):].any()                                     # empty slots: 0
    print("worst error / scale (bound %.2e):" % TOL, {k: "%.2e" % v for k, v in worst.items()})


def test_accumulate_form_is_the_write_form_plus_an_fp32_add(tables):
    for n, (t, _) in enumerate(tables[::4] + tables[-2:]):
        g = torch.Generator().manual_seed(n)
        pre = tuple(torch.randn(t[k].shape, generator=g).to(DEV) for k in ("center", "size", "angle"))
        acc = _bwd(t, into=tuple(p.clone() for p in pre))
        written = _bwd(t)
        matched = _matched_rows(t).to(DEV)
        for a, p, w in zip(acc, pre, written):
            assert _same_bits(a, torch.add(p, w))
            assert _same_bits(a[~matched], p[~matched])                           # untouched, not "plus zero"
            assert not _same_bits(a, p) or not bool(matched.any())


def test_upstream_gradient_scales_the_write_form_exactly(tables):
    t, _ = tables[0]
    one = _bwd(t)
    explicit = _bwd(t, gout=torch.tensor(1.0, device=DEV))
    half = _bwd(t, gout=torch.tensor(0.5, device=DEV))
    for a, e, h in zip(one, explicit, half):
        assert _same_bits(a, e)
        assert _same_bits(h, a * 0.5) and bool(a.any())


def test_two_launches_give_the_same_bits(tables):
    for t, _ in (tables[0], tables[-1]):
        first, second = _fwd(t), _fwd(t)
        for a, b in zip(first, second):
            assert _same_bits(a, b)
        for a, b in zip(_bwd(t), _bwd(t)):
            assert _same_bits(a, b)


# ----------------------------------------------------------------------------------------------------------------------- Loss
BASE = {"total_class": 1.0, "object_class": 0.5, "center": 1.0, "size": 2.0, "angle": 1.0}


def _loss(weights, on_device):
    from dpft_amd.training.loss import Loss
    loss = Loss.from_config({"anassigner": "HungarianAnassigner", "criterion": "SetCriterion", "loss_weights": dict(weights),
                             "reduction": "mean"})
    loss.assign_on_device = on_device
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


def _run(weights, on_device, counts, seed):
    loss = _loss(weights, on_device)
    out, labels = _outputs(seed), _labels(counts, seed + 50)
    total, losses = loss(out, labels)
    last = loss.__dict__["_last"]
    table = {"center": last[1], "size": last[2], "angle": last[3], "gt_box": last[4], "match": last[6], "counts": last[7]}
    total.backward()
    loss.check_assignment_status()
    return total.detach(), {k: v.detach() for k, v in losses.items()}, {k: v.grad for k, v in out.items()}, table


@pytest.mark.parametrize("counts", [(3, 0), (1, 4)])
def test_loss_adds_the_term_to_an_unchanged_five_term_criterion(counts, monkeypatch):
    from dpft_amd.hip.lib import lib
    cost_weights, orig = [], lib.call

    def recording(name, *args):
        if name == "dpft_match_cost_f32":
            cost_weights.append(tuple(args[7]._obj))
        return orig(name, *args)
    monkeypatch.setattr(lib, "call", recording)
    runs = {}
    for on_device in (False, True):
        twin_total, twin_losses, twin_grads, _ = _run(BASE, on_device, counts, seed=3)
        total, losses, grads, table = _run({**BASE, "giou": W}, on_device, counts, seed=3)
        assert list(losses) == list(BASE) + ["giou"] and list(twin_losses) == list(BASE)
        for k in BASE:
            assert _same_bits(losses[k], twin_losses[k]), k
        term = losses["giou"]
        assert 0.0 <= float(term) <= W and float(term) > 0.0
        assert _same_bits(total, twin_total + term)                                  # one fp32 add
        kernel = _bwd({**table, "where": None}, w=W)
        for k, extra in zip(("center", "size", "angle"), kernel):
            assert _same_bits(grads[k], twin_grads[k] + extra), k
            assert bool(extra.any())
        assert _same_bits(grads["class"], twin_grads["class"])
        ref_term, _, _ = _fwd(table, w=W, total_in=float(twin_total))
        assert _same_bits(ref_term, term)
        runs[on_device] = (total, losses, grads)
    for a, b in zip(runs[False][2].values(), runs[True][2].values()):
        assert _same_bits(a, b)
    assert _same_bits(runs[False][0], runs[True][0]) and _same_bits(runs[False][1]["giou"], runs[True][1]["giou"])
    # the matcher's cost weights: its four keys and giou_weight = 1.0 -- the criterion's "giou" weight does not reach them
    assert len(cost_weights) == 4 and set(cost_weights) == {(1.0, 1.0, 2.0, 1.0, 1.0)}


def test_loss_without_any_target_is_zero_and_still_names_the_term():
    loss = _loss({**BASE, "giou": W}, True)
    total, losses = loss(_outputs(5), _labels((0, 0), 5))
    assert float(total.detach()) == 0.0 and list(losses) == list(BASE) + ["giou"] and float(losses["giou"].detach()) == 0.0
    assert loss.last_has_targets is False
    total.backward()


def test_backward_into_adds_the_term_behind_the_five_term_gradient():
    """The trainer's direct chain without buffers named in advance: dpft_set_loss_bwd_f32 writes, the GIoU backward adds."""
    loss = _loss({**BASE, "giou": W}, True)
    out, labels = _outputs(7), _labels((2, 3), 57)
    total, _ = loss(out, labels)
    keys = ("center", "size", "angle", "class")
    bufs = [torch.full_like(out[k], float("nan")) for k in keys]
    assert loss.backward_into(total, *bufs)
    total2, _ = loss(out, labels)
    total2.backward()
    for k, b in zip(keys, bufs):
        assert _same_bits(b, out[k].grad), k


def test_loss_under_no_grad_runs_the_forward_entry_only(monkeypatch):
    from dpft_amd.hip.lib import lib
    names, orig = [], lib.call

    def recording(name, *args):
        names.append(name)
        return orig(name, *args)
    monkeypatch.setattr(lib, "call", recording)
    loss = _loss({**BASE, "giou": W}, True)
    with torch.no_grad():
        total, losses = loss(_outputs(6), _labels((2, 3), 6))
    assert [n for n in names if "giou_loss" in n] == ["dpft_giou_loss_fwd_f32"]
    assert not total.requires_grad and float(losses["giou"]) > 0


def test_loss_under_no_grad_leaves_named_gradient_buffers_to_the_five_terms(monkeypatch):
    """fused_grad_targets named on a stand-alone Loss under no_grad: the GIoU backward is not launched into the caller's buffers
    (they hold what a twin without the key leaves there), and a backward_into() into them afterwards writes the whole gradient."""
    from dpft_amd.hip.lib import lib
    names, orig = [], lib.call

    def recording(name, *args):
        names.append(name)
        return orig(name, *args)
    monkeypatch.setattr(lib, "call", recording)
    keys = ("center", "size", "angle", "class")
    left = {}
    for tag, weights in (("twin", BASE), ("giou", {**BASE, "giou": W})):
        loss = _loss(weights, True)
        out, labels = _outputs(8), _labels((2, 3), 58)
        bufs = tuple(torch.full_like(out[k], float("nan")) for k in keys)
        loss.fused_grad_targets = bufs
        with torch.no_grad():
            total, _ = loss(out, labels)
        left[tag] = [b.clone() for b in bufs]
    assert [n for n in names if "giou_loss" in n] == ["dpft_giou_loss_fwd_f32"]
    for a, b in zip(left["twin"], left["giou"]):
        assert _same_bits(a, b) and bool(torch.isfinite(a).all())
    assert loss.backward_into(total, *bufs)
    loss.fused_grad_targets = None
    total2, _ = loss(out, labels)
    total2.backward()
    for k, b in zip(keys, bufs):
        assert _same_bits(b, out[k].grad), k


# -------------------------------------------------------------------------------------------------------------------- trainer
SHAPES = {"camera_mono": (96, 160, 3), "radar_bev": (128, 43, 6), "radar_front": (37, 107, 6)}
NEW_ENTRIES = {"dpft_giou_loss_fwd_f32", "dpft_giou_loss_bwd_f32"}


def _trainer(giou):
    from dpft_amd.configs import load_config
    from dpft_amd.models import build
    from dpft_amd.synthetic import make_batch, make_labels
    from dpft_amd.training.trainer import DataParallelTrainer
    cfg = copy.deepcopy(load_config("kradar"))
    cfg["model"]["backbones"]["camera_mono"]["name"] = "ResNet50"
    cfg["model"]["fuser"]["dropout"] = 0.0
    if giou is not None:
        cfg["train"]["loss_weights"]["giou"] = giou
    batch = make_batch(cfg["model"]["inputs"], 2, seed=9, shapes=SHAPES, device=DEV)
    labels = make_labels(2, seed=9, device=DEV)
    torch.manual_seed(0)
    tr = DataParallelTrainer(build("dprt", cfg), cfg, torch.device(DEV))
    tr.enable_graphs(batch)
    return tr, batch, labels


def _entry_names(monkeypatch, fn):
    """Names of the new C entries that pass through lib.call while fn() runs."""
    from dpft_amd.hip.lib import lib
    names, orig = [], lib.call

    def recording(name, *args):
        names.append(name)
        return orig(name, *args)
    with monkeypatch.context() as m:
        m.setattr(lib, "call", recording)
        fn()
    return [n for n in names if n in NEW_ENTRIES]


def test_trainer_without_the_key_launches_neither_new_entry(monkeypatch):
    tr, batch, labels = _trainer(None)
    tr.train_step(batch, labels)
    called = _entry_names(monkeypatch, lambda: tr.train_step(batch, labels))
    assert called == []
    _, losses = tr.train_step(batch, labels)
    assert "giou" not in losses
    assert _entry_names(monkeypatch, lambda: tr.validate_one_epoch(0, [(batch, labels)])) == []


def test_trainer_step_with_the_term(monkeypatch):
    from dpft_amd.hip.lib import lib, stream
    tr, batch, labels = _trainer(W)
    loss, losses = tr.train_step(batch, labels)
    assert "giou" in losses and torch.isfinite(losses["giou"]) and 0.0 <= float(losses["giou"]) <= W
    g = tr.model.__dict__.get("_graphed_fuser")
    assert g is not None, "the test is about the replayed decoder's static gradient buffers"
    # what the loss call leaves in the decoder graph's static gradient buffers, and the inputs it had
    seen = {}
    forward = tr.loss_fn.forward

    def spying(output, lab):
        res = forward(output, lab)
        assert tr.loss_fn.__dict__.get("fused_grad_targets") is not None
        seen["bufs"] = [t.clone() for t in g.static_grad_outputs[:4]]
        seen["last"] = [t.clone() if isinstance(t, torch.Tensor) else t for t in tr.loss_fn.__dict__["_last"]]
        return res
    with monkeypatch.context() as m:
        m.setattr(tr.loss_fn, "forward", spying)
        called = _entry_names(monkeypatch, lambda: tr.train_step(batch, labels))
    assert called == ["dpft_giou_loss_fwd_f32", "dpft_giou_loss_bwd_f32"]               # once each per step
    cls, center, size, angle, gt_box, gt_onehot, match, counts, weights5, alpha, sel, _ = seen["last"]
    B, N, ncls = cls.shape
    five = [torch.empty_like(t) for t in (center, size, angle, cls)]
    w5 = (C.c_float * 5)(*weights5)
    lib.call("dpft_set_loss_bwd_f32", cls.data_ptr(), center.data_ptr(), size.data_ptr(), angle.data_ptr(), gt_box.data_ptr(),
             gt_onehot.data_ptr(), match.data_ptr(), counts.data_ptr(), C.byref(w5), alpha, sel.data_ptr(), five[3].data_ptr(),
             five[0].data_ptr(), five[1].data_ptr(), five[2].data_ptr(), B, N, gt_box.shape[1], ncls, stream())
    table = {"center": center, "size": size, "angle": angle, "gt_box": gt_box, "match": match, "counts": counts}
    extra = _bwd(table, w=W)
    for k in range(3):
        assert _same_bits(seen["bufs"][k], five[k] + extra[k]), k
    assert _same_bits(seen["bufs"][3], five[3])
    # validation: the forward entry alone
    assert _entry_names(monkeypatch, lambda: tr.validate_one_epoch(0, [(batch, labels)])) == ["dpft_giou_loss_fwd_f32"]
