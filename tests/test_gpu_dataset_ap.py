"""Split-level AP_BEV / AP_3D on the device (csrc/dataset_ap.hip, dpft_amd/evaluation/dataset_ap.py) against the fp64
restatement of tests/dataset_ap_ref.py.  The records are read back, brought to the reference's order and must equal the
reference's (score bits, frame, query, class, TP bits) bit for bit; npos, the TP totals and dropped_nan must be equal; ap may
differ by 1e-12 (at most 101 fp64 terms in [0, 1], each a correctly rounded quotient of exact integers)."""
import copy
import os

import numpy as np
import pytest
import torch

from tests import dataset_ap_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
AP_TOL = 1e-12


def _batch(samples):
    out = {k: torch.from_numpy(np.stack([s[src] for s in samples])).to(DEV)
           for k, src in (("class", "cls"), ("center", "center"), ("size", "size"), ("angle", "angle"))}
    labels = [{k: torch.from_numpy(s[k]).to(DEV) for k in ("gt_center", "gt_size", "gt_angle", "gt_class")} for s in samples]
    return out, labels


def _feed(ap, frames):
    """One update per run of consecutive frame indices."""
    i = 0
    while i < len(frames):
        j = i + 1
        while j < len(frames) and frames[j][0] == frames[j - 1][0] + 1:
            j += 1
        out, labels = _batch([s for _, s in frames[i:j]])
        ap.update(out, labels, frames[i][0])
        i = j


def _records(ap):
    """The store's records in the reference's order and layout, sorted here (numpy) from the raw state."""
    rec = ap.state()["records"].cpu().numpy()
    score = rec[:, 0].copy().view(np.float32).astype(np.float64)
    cols = np.stack([rec[:, 0], rec[:, 1], rec[:, 2] & 0xFFFF, (rec[:, 2] >> 16) & 0xFF, rec[:, 3]], 1).astype(np.int64)
    return cols[np.lexsort((cols[:, 2], cols[:, 1], -score, cols[:, 3]))]


def _same(a, b, tol=0.0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= tol)))


def _same_dict(a, b):
    return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)


def _check(ap, ref):
    got = _records(ap)
    assert got.shape == ref["records"].shape, (got.shape, ref["records"].shape)
    assert np.array_equal(got, ref["records"]), np.argwhere(got != ref["records"])[:5]
    res = ap.compute()
    assert _same(res["npos"], ref["npos"]) and _same(res["tp"], ref["tp"]), (res["npos"], ref["npos"], res["tp"], ref["tp"])
    assert res["dropped_nan"] == ref["dropped_nan"]
    err = np.nanmax(np.abs(res["ap"].numpy() - ref["ap"]), initial=0.0)
    print("max |ap - ref| =", err)
    assert _same(res["ap"], ref["ap"], AP_TOL), err
    for k, (kind, thr) in enumerate(ref["combos"]):
        assert _same(res[f"mAP_{kind}@{thr:g}"], ref["mAP"][k], AP_TOL)
        for c in range(1, ap.num_classes):
            assert _same(res[f"AP_{kind}@{thr:g}/{c}"], ref["ap"][c - 1, k], AP_TOL)
    for c in range(1, ap.num_classes):
        assert res[f"npos/{c}"] == ref["npos"][c - 1]
    return res


def _new(C, params, **kw):
    from dpft_amd.evaluation.dataset_ap import DatasetAP
    return DatasetAP(C, **params, **kw)


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_records_and_table_equal_the_reference_over_the_shapes(name):
    frames, C, params, ref = R.shape_case(name)
    ap = _new(C, params)
    _feed(ap, frames)
    _check(ap, ref)


@pytest.mark.parametrize("name", sorted(R.directed_cases()))
def test_directed_cases(name):
    frames, C, params, _ties = R.directed_cases()[name]
    ref = R.run(frames, C, **params)
    ap = _new(C, params)
    _feed(ap, frames)
    res = _check(ap, ref)
    if name == "strict":      # IoU exactly 0.5: not matched at 0.5, matched at 0.3 (bev@0.3, bev@0.5, 3d@0.3, 3d@0.5)
        assert res["ap"][0].tolist() == [1.0, 0.0, 1.0, 0.0] and _records(ap)[0, 4] == 0b0101
    if name == "all_background":
        assert _records(ap).shape == (0, 5) and res["npos/1"] == 1.0 and res["AP_bev@0.3/1"] == 0.0
    if name == "nan_score":
        assert res["dropped_nan"] == 2.0


def _stream_batches(sizes):
    frames, C, params, ref = R.stream_case()
    assert sum(sizes) == len(frames)
    out, i = [], 0
    for s in sizes:
        out.append(frames[i:i + s])
        i += s
    return out, C, params, ref


def test_updates_growing_the_store_equal_one_update_of_the_concatenation():
    """7 updates of unequal batch size from a store of 64 records (one frame has 65 queries): it doubles five times; the result is
    that of ONE update with all 16 frames, and that of the reference."""
    batches, C, params, ref = _stream_batches([1, 3, 2, 1, 4, 2, 3])
    ap = _new(C, params, initial_capacity=64)
    caps = []
    for b in batches:
        _feed(ap, b)
        caps.append(ap.capacity)
    assert caps[0] == 128 and caps[-1] == 2048 and len(set(caps)) >= 3, caps
    _check(ap, ref)
    whole = _new(C, params)
    _feed(whole, [f for b in batches for f in b])
    assert whole.capacity == 1 << 16
    _check(whole, ref)
    assert np.array_equal(_records(ap), _records(whole))
    assert torch.equal(ap.compute()["ap"], whole.compute()["ap"])


def test_merge_order_and_reset():
    batches, C, params, ref = _stream_batches([5, 3, 4, 4])
    # merge of two halves = the whole
    a, b = _new(C, params, initial_capacity=64), _new(C, params)
    for x in batches[:2]:
        _feed(a, x)
    for x in batches[2:]:
        _feed(b, x)
    a.merge(b)
    _check(a, ref)
    # the updates issued in another order, with the same first_frame values
    c = _new(C, params, initial_capacity=256)
    for x in (batches[2], batches[0], batches[3], batches[1]):
        _feed(c, x)
    _check(c, ref)
    assert torch.equal(c.compute()["ap"], a.compute()["ap"])
    # state() / load_state() carry everything
    d = _new(C, params)
    d.load_state(c.state())
    _check(d, ref)
    # reset() leaves nothing behind
    c.reset()
    assert c.capacity == 0 and c.state()["records"].shape == (0, 4) and int(c.state()["counters"].sum()) == 0
    _feed(c, batches[1])
    _check(c, R.run(batches[1], C, **params))
    # merging into an empty accumulator
    e = _new(C, params)
    e.merge(d)
    _check(e, ref)
    # frame indices are int32 in the records
    for bad in (-1, 1 << 31):
        with pytest.raises(ValueError, match="first_frame"):
            e.update(*_batch([batches[0][0][1]]), bad)
    _check(e, ref)


def test_update_does_not_make_the_host_wait():
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch has no torch.cuda.set_sync_debug_mode")
    batches, C, params, ref = _stream_batches([1, 3, 2, 1, 4, 2, 3])
    ap = _new(C, params, initial_capacity=64)
    fed = [_batch([s for _, s in b]) for b in batches]
    torch.cuda.synchronize()
    try:
        for i, (b, (out, labels)) in enumerate(zip(batches, fed)):
            if i == 2:
                torch.cuda.set_sync_debug_mode("error")
            ap.update(out, labels, b[0][0])                 # (grows the store on the way: 128 -> 2048 records)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _check(ap, ref)


# ------------------------------------------------------------------------------------------------- the public interface
class _Stub(torch.nn.Module):
    """A 'model' that returns precomputed head outputs: data['idx'] selects the frames of the batch."""

    def __init__(self, frames):
        super().__init__()
        self.out, _ = _batch([s for _, s in frames])
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward(self, data):
        return {k: v[data["idx"]] for k, v in self.out.items()}


def _loader(frames, bs):
    batches = []
    for i in range(0, len(frames), bs):
        chunk = frames[i:i + bs]
        _, labels = _batch([s for _, s in chunk])
        for k, lab in enumerate(labels):
            lab["description"] = torch.tensor([(i + k) % 8, (i + k) % 2, (i + k) % 7])
        batches.append(({"idx": torch.arange(i, i + len(chunk))}, labels))
    return batches


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            out[os.path.relpath(os.path.join(d, f), root)] = open(os.path.join(d, f)).read()
    return out


class _Writer:
    def __init__(self):
        self.tags = {}

    def add_scalar(self, tag, value, step):
        self.tags[tag] = (value, step)


@pytest.mark.parametrize("logging", ["epoch", "step"])
def test_evaluate_one_epoch_returns_the_split_table_and_nothing_else_changes(tmp_path, logging):
    from dpft_amd.evaluation import DataParallelEvaluator, Metric
    from dpft_amd.evaluation.exporters.kradar import KRadarExporter
    frames, C, params, ref = R.stream_case()
    model, loader = _Stub(frames).to(DEV), _loader(frames, 3)

    def evaluator(ap):
        return DataParallelEvaluator(metric=Metric(metrics={"mAP": "mAP3D", "mGIoU": "mGIoU3D"}),
                                     exporter=KRadarExporter(conf_thrs=[0.0, 0.5]), device=torch.device(DEV), logging=logging,
                                     dataset_ap=ap)
    w0, w1 = _Writer(), _Writer()
    plain = evaluator(None).evaluate_one_epoch(2, model, loader, w0, str(tmp_path / "plain"), shard_start=frames[0][0])
    assert set(plain) == {"mAP", "mGIoU"}                                   # what it returns today
    ap = _new(C, params)
    got = evaluator(ap).evaluate_one_epoch(2, model, loader, w1, str(tmp_path / "with"), shard_start=frames[0][0])
    assert _same_dict({k: v for k, v in got.items() if k in plain}, plain)
    t0, t1 = _tree(str(tmp_path / "plain")), _tree(str(tmp_path / "with"))
    assert t0 and t0 == t1
    extra = set(got) - set(plain)
    names = [f"{kind}@{thr:g}" for kind, thr in ref["combos"]]
    assert extra == {f"mAP_{n}" for n in names} | {f"AP_{n}/{c}" for n in names for c in range(1, C)} | \
        {f"npos/{c}" for c in range(1, C)} | {"dropped_nan"}
    for k, n in enumerate(names):
        assert _same(got[f"mAP_{n}"], ref["mAP"][k], AP_TOL), (n, got[f"mAP_{n}"], ref["mAP"][k])
    _check(ap, ref)
    # logged under test/ at the end of the epoch, in both logging modes; the plain run logs what it always did
    step = 2 if logging == "epoch" else 3 * len(loader) - 1
    assert all(w1.tags[f"test/{k}"][1] == step for k in extra)
    assert set(w1.tags) - set(w0.tags) == {f"test/{k}" for k in extra}
    # a second epoch starts from an empty store
    again = evaluator(ap).evaluate_one_epoch(3, model, loader, None, None, shard_start=frames[0][0])
    assert _same_dict(again, got)


def test_from_config_builds_it_only_with_the_key():
    from dpft_amd.configs import load_config
    from dpft_amd.evaluation import DataParallelEvaluator
    cfg = copy.deepcopy(load_config("kradar"))
    assert DataParallelEvaluator.from_config(cfg).dataset_ap is None
    cfg["evaluate"]["dataset_ap"] = {"iou": [0.5], "recall_points": 11}
    ap = DataParallelEvaluator.from_config(cfg).dataset_ap
    assert ap.num_classes == 2 and ap.combinations == [("bev", 0.5), ("3d", 0.5)] and ap.recall_points == 11


class _StubLoss(torch.nn.Module):
    def forward(self, output, labels):
        loss = (output["center"] ** 2).mean()
        return loss, {"center": loss}


@pytest.mark.parametrize("key", [None, {"iou": [0.3, 0.5, 0.7], "recall_points": 40}])
def test_trainer_validation_adds_the_table_only_with_the_key(key):
    from dpft_amd.configs import load_config
    from dpft_amd.training.trainer import DataParallelTrainer
    frames, C, params, ref = R.stream_case()
    cfg = copy.deepcopy(load_config("kradar"))
    cfg["train"]["optimizer"] = {"name": "AdamW", "lr": 1e-2}
    cfg["model"]["head"]["num_classes"] = C
    cfg["evaluate"] = {} if key is None else {"dataset_ap": key}
    tr = DataParallelTrainer(_Stub(frames), cfg, torch.device(DEV))
    tr.loss_fn = _StubLoss()
    w = _Writer()
    res = tr.validate_one_epoch(1, _loader(frames, 5), w)
    names = [f"{kind}@{thr:g}" for kind, thr in ref["combos"]]
    if key is None:
        assert tr.dataset_ap is None and set(res) == {"loss", "loss_center"} and set(w.tags) == {"val/loss", "val/loss_center"}
        return
    assert set(res) == {"loss", "loss_center", "dropped_nan"} | {f"mAP_{n}" for n in names} | \
        {f"AP_{n}/{c}" for n in names for c in range(1, C)} | {f"npos/{c}" for c in range(1, C)}
    for k, n in enumerate(names):      # frames are numbered rank * 2^24 + local index: the same order as the reference's
        assert _same(res[f"mAP_{n}"], ref["mAP"][k], AP_TOL)
    assert all(f"val/mAP_{n}" in w.tags for n in names) and w.tags["val/npos/1"] == (ref["npos"][0], 1)
    assert _same_dict(tr.validate_one_epoch(2, _loader(frames, 5), None), res)      # reset at the start of every epoch
