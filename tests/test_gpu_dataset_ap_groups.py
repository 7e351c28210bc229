"""Split-level AP per scene-description group on the device (evaluate.dataset_ap.groups: dpft_dataset_ap_update_groups_f32,
dpft_dataset_ap_finalize_groups_f64) against the fp64 restatement of tests/dataset_ap_groups_ref.py, by the rule
tests/test_gpu_dataset_ap.py applies to the ungrouped table: npos, the TP totals, nframes and bad_description must be equal, ap may
differ by 1e-12 (at most 101 fp64 terms in [0, 1], each a correctly rounded quotient of exact integers).  Against an UNGROUPED
accumulator fed a group's frames alone there is no tolerance: the same integers go through the same fp64 expressions.

The shapes are the smallest at which the grouped scan can go wrong: the stream case has 32 frames whose time of day flips with every
frame and 522 records in one class (membership flips inside every wave and across two 256-record trip boundaries); the shape cases
have groups without a frame, groups of one frame, classes without ground truth in a group, updates of 1 and 3 frames, K = 1 and 8,
C = 2 and 16, R = 2, 40 and 101, one axis, two axes and all three; the missed-class case has ground truth without a detection."""
import copy
import threading

import numpy as np
import pytest
import torch
import torch.distributed

from tests import dataset_ap_groups_ref as G
from tests import dataset_ap_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
AP_TOL = 1e-12
# how a frame's description reaches update(): device tensors travel as pointers, host tensors as values
STORAGES = {"dev_f32": (torch.float32, DEV), "dev_f64": (torch.float64, DEV), "dev_i32": (torch.int32, DEV),
            "dev_i64": (torch.int64, DEV), "host_f32": (torch.float32, "cpu"), "host_f64": (torch.float64, "cpu"),
            "host_i64": (torch.int64, "cpu")}


def _batch(samples, descriptions=None, storage="dev_f32"):
    out = {k: torch.from_numpy(np.stack([s[src] for s in samples])).to(DEV)
           for k, src in (("class", "cls"), ("center", "center"), ("size", "size"), ("angle", "angle"))}
    labels = [{k: torch.from_numpy(s[k]).to(DEV) for k in ("gt_center", "gt_size", "gt_angle", "gt_class")} for s in samples]
    if descriptions is not None:
        dtype, where = STORAGES[storage]
        for lab, d in zip(labels, descriptions):
            lab["description"] = torch.from_numpy(np.asarray(d)).to(dtype).to(where)
    return out, labels


def _feed(ap, frames, descriptions=None, storage="dev_f32", only=None):
    """One update per run of consecutive frame indices (of the frames at the positions ``only``, when given)."""
    pos = list(range(len(frames))) if only is None else list(only)
    i = 0
    while i < len(pos):
        j = i + 1
        while j < len(pos) and frames[pos[j]][0] == frames[pos[j - 1]][0] + 1:
            j += 1
        out, labels = _batch([frames[p][1] for p in pos[i:j]], None if descriptions is None else [descriptions[p] for p in pos[i:j]],
                             storage)
        ap.update(out, labels, frames[pos[i]][0])
        i = j


def _same(a, b, tol=0.0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= tol)))


def _bits(t):
    return torch.as_tensor(t, dtype=torch.float64).contiguous().view(torch.int64)


def _new(C, params, **kw):
    from dpft_amd.evaluation.dataset_ap import DatasetAP
    return DatasetAP(C, **params, **kw)


def _check(ap, ref):
    """Every group's table against the reference, tensors and scalar keys alike."""
    res = ap.compute()
    assert res["group_names"] == ref["names"] and res["group_names"][0] == "all"
    assert _same(res["group_npos"], ref["npos"]) and _same(res["group_tp"], ref["tp"]), (res["group_npos"], ref["npos"])
    assert _same(res["group_nframes"], ref["nframes"]), (res["group_nframes"], ref["nframes"])
    assert res["bad_description"] == ref["bad_description"] and res["dropped_nan"] == ref["dropped_nan"]
    err = np.nanmax(np.abs(res["group_ap"].numpy() - ref["ap"]), initial=0.0)
    print("max |group_ap - ref| =", err)
    assert _same(res["group_ap"], ref["ap"], AP_TOL), err
    C = ap.num_classes
    for g, name in enumerate(ref["names"]):
        tail = "" if g == 0 else "/" + name
        for k, (kind, thr) in enumerate(ref["combos"]):
            assert _same(res[f"mAP_{kind}@{thr:g}{tail}"], ref["mAP"][g, k], AP_TOL), (name, kind, thr)
            for c in range(1, C):
                assert _same(res[f"AP_{kind}@{thr:g}/{c}{tail}"], ref["ap"][g, c - 1, k], AP_TOL)
        for c in range(1, C):
            assert res[f"npos/{c}{tail}"] == ref["npos"][g, c - 1]
        if g:
            assert res[f"nframes/{name}"] == ref["nframes"][g]
    assert "nframes/all" not in res and "nframes" not in res
    return res


def _twins(res, frames, C, params, ref):
    """Every group's table equals, bit for bit, an ungrouped accumulator fed only that group's frames."""
    for g, name in enumerate(ref["names"]):
        twin = _new(C, params)
        _feed(twin, frames, only=ref["members"][name])
        t = twin.compute()
        for mine, theirs in (("group_ap", "ap"), ("group_tp", "tp"), ("group_npos", "npos")):
            assert torch.equal(_bits(res[mine][g]), _bits(t[theirs])), (name, mine, res[mine][g], t[theirs])


def _case(name):
    if name == "stream":
        frames, descriptions, C, params, ref = G.stream_case()
        assert G.conditions(frames, descriptions, C, params, ref) == []
        return frames, descriptions, C, params, True, ref
    if name == "missed_class":
        frames, descriptions, C, params, ref = G.missed_class_case()
        fog = ref["names"].index("weather=fog")
        assert ref["npos"][fog, 1] == 1 and ref["nrec"][fog, 1] == 0 and np.all(ref["ap"][fog, 1] == 0)
        return frames, descriptions, C, params, True, ref
    frames, descriptions, C, params, groups, ref = G.shape_case(name)
    assert R.violations(frames, C, params) == [] and (ref["nframes"] == 0).any() and (ref["nframes"] == 1).any()
    assert ((ref["npos"] == 0) & (ref["nframes"][:, None] > 0)).any() and [f for f, _ in frames][:4] == [11, 14, 15, 16]
    return frames, descriptions, C, params, groups, ref


CASES = ["stream", "missed_class"] + sorted(G.SHAPES)


@pytest.mark.parametrize("name, storage", list(zip(CASES, ["dev_f32", "host_f32", "dev_i64", "dev_i32", "host_i64"])))
def test_every_group_equals_the_reference_and_its_ungrouped_twin(name, storage):
    frames, descriptions, C, params, groups, ref = _case(name)
    ap = _new(C, params, groups=groups)
    _feed(ap, frames, descriptions, storage)
    res = _check(ap, ref)
    _twins(res, frames, C, params, ref)


def test_the_all_group_and_todays_keys_are_those_of_an_accumulator_without_groups():
    frames, descriptions, C, params, _, ref = _case("stream")
    plain, grouped = _new(C, params), _new(C, params, groups=True)
    _feed(plain, frames)
    _feed(grouped, frames, descriptions)
    a, b = plain.compute(), grouped.compute()
    assert set(a) < set(b) and "frames" not in plain.state() and set(grouped.state()) == {"records", "counters", "frames"}
    for k, v in a.items():
        assert torch.equal(_bits(v), _bits(b[k])), k
    for mine, theirs in (("group_ap", "ap"), ("group_tp", "tp"), ("group_npos", "npos")):
        assert torch.equal(_bits(b[mine][0]), _bits(a[theirs])), mine
    # the records are the ungrouped ones bit for bit (the same launches write them)
    ra, rb = (x.state()["records"].cpu().numpy() for x in (plain, grouped))
    key = lambda r: np.lexsort((r[:, 2], r[:, 1]))
    assert np.array_equal(ra[key(ra)], rb[key(rb)])
    assert torch.equal(plain.state()["counters"], grouped.state()["counters"])


@pytest.mark.parametrize("storage", ["dev_f64", "host_f64", "dev_f32"])
def test_bad_descriptions_count_in_all_only(storage):
    """-1, 9, time 2, weather 7, NaN and infinities leave the frame without a group on that axis; -0.5, 1.9 and 6.999 truncate into
    the table the way int() does."""
    frames, descriptions, C, params, ref = G.bad_case()
    assert ref["bad_description"] == 9 and ref["nframes"][0] == 12
    ap = _new(C, params, groups=True)
    _feed(ap, frames, descriptions, storage)
    res = _check(ap, ref)
    for axis, bad in ref["bad_per_axis"].items():
        mine = [g for g, n in enumerate(ref["names"]) if n.startswith(axis + "=")]
        assert float(res["group_nframes"][mine].sum()) == 12 - len(bad)
    assert res["nframes/time=night"] == ref["nframes"][ref["names"].index("time=night")]
    _twins(res, frames, C, params, ref)


def _stream_batches(sizes):
    frames, descriptions, C, params, _, ref = _case("stream")
    assert sum(sizes) == len(frames)
    out, i = [], 0
    for s in sizes:
        out.append(list(range(i, i + s)))
        i += s
    return out, frames, descriptions, C, params, ref


def test_updates_growing_both_stores_equal_one_accumulation_of_the_concatenation():
    batches, frames, descriptions, C, params, ref = _stream_batches([1, 3, 2, 1, 4, 2, 3, 5, 1, 6, 4])
    ap = _new(C, params, groups=True, initial_capacity=64, initial_frame_capacity=1)
    caps = []
    for b in batches:
        _feed(ap, frames, descriptions, only=b)
        caps.append((ap.capacity, ap.frame_capacity))
    assert caps[0] == (128, 1) and caps[-1] == (4096, 32) and len({c for c, _ in caps}) >= 4 and len({f for _, f in caps}) == 5, caps
    res = _check(ap, ref)
    whole = _new(C, params, groups=True)
    _feed(whole, frames, descriptions)
    assert (whole.capacity, whole.frame_capacity) == (1 << 16, 1 << 10)
    w = _check(whole, ref)
    for k in ("group_ap", "group_tp", "group_npos", "group_nframes"):
        assert torch.equal(_bits(res[k]), _bits(w[k])), k


class _PlayedRanks:
    """torch.distributed's collectives for ranks played by threads of this process: every rank deposits its tensor, all wait, all
    read."""

    def __init__(self, world):
        self.world, self.local = world, threading.local()
        self.slots, self.barrier = [None] * world, threading.Barrier(world)

    def get_world_size(self):
        return self.world

    def _exchange(self, t):
        self.slots[self.local.rank] = t
        self.barrier.wait(60)
        got = [s.clone() for s in self.slots]
        self.barrier.wait(60)
        return got

    def all_gather(self, out, t):
        for o, s in zip(out, self._exchange(t)):
            o.copy_(s)

    def all_reduce(self, t, op=None):
        assert op == torch.distributed.ReduceOp.SUM
        t.copy_(sum(self._exchange(t)))


def test_merge_load_state_and_two_played_ranks_give_the_single_accumulator_table(monkeypatch):
    from dpft_amd.evaluation.dataset_ap import gather_state
    batches, frames, descriptions, C, params, ref = _stream_batches([5, 3, 4, 4, 7, 9])
    halves = []
    for part in (batches[:3], batches[3:]):
        ap = _new(C, params, groups=True, initial_capacity=64, initial_frame_capacity=2)
        for b in part:
            _feed(ap, frames, descriptions, only=b)
        halves.append(ap)
    single = _new(C, params, groups=True)
    _feed(single, frames, descriptions)
    want = _check(single, ref)

    def equal(ap):
        got = _check(ap, ref)
        return all(torch.equal(_bits(got[k]), _bits(want[k])) for k in ("group_ap", "group_tp", "group_npos", "group_nframes"))
    # state() / load_state() carry the frame rows
    st = [h.state() for h in halves]
    assert [int(s["frames"].shape[0]) for s in st] == [12, 20] and st[0]["frames"].shape[1] == 18
    loaded = _new(C, params, groups=True)
    loaded.load_state(single.state())
    assert equal(loaded)
    with pytest.raises(ValueError, match="frames"):
        loaded.load_state({k: v for k, v in single.state().items() if k != "frames"})
    # two ranks played by two threads through gather_state: both end up with the single accumulator's table
    played, out = _PlayedRanks(2), [None, None]
    for name in ("get_world_size", "all_gather", "all_reduce"):
        monkeypatch.setattr(torch.distributed, name, getattr(played, name))

    def rank(r):
        played.local.rank = r
        out[r] = gather_state(st[r])
    threads = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    monkeypatch.undo()
    for r in range(2):
        assert out[r] is not None and int(out[r]["frames"].shape[0]) == 32
        ap = _new(C, params, groups=True)
        ap.load_state(out[r])
        assert equal(ap)
    # merge: the second half into the first, into an empty accumulator, and the refusal of other groups
    halves[0].merge(halves[1])
    assert equal(halves[0])
    empty = _new(C, params, groups=True)
    empty.merge(single)
    assert equal(empty)
    with pytest.raises(ValueError, match="differ"):
        empty.merge(_new(C, params, groups=["time"]))
    with pytest.raises(ValueError, match="differ"):
        empty.merge(_new(C, params))
    # reset() leaves no frame behind
    empty.reset()
    assert empty.frame_capacity == 0 and empty.state()["frames"].shape == (0, 18)
    assert empty.compute()["group_nframes"].sum() == 0


@pytest.mark.parametrize("storage", ["dev_f32", "host_f32"])
def test_update_with_groups_does_not_make_the_host_wait(storage):
    batches, frames, descriptions, C, params, ref = _stream_batches([1, 3, 2, 1, 4, 2, 3, 5, 1, 6, 4])
    ap = _new(C, params, groups=True, initial_capacity=64, initial_frame_capacity=1)
    fed = [_batch([frames[p][1] for p in b], [descriptions[p] for p in b], storage) for b in batches]
    torch.cuda.synchronize()
    try:
        for i, (b, (out, labels)) in enumerate(zip(batches, fed)):
            if i == 2:
                torch.cuda.set_sync_debug_mode("error")
            ap.update(out, labels, frames[b[0]][0])             # (grows both stores on the way)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _check(ap, ref)


def test_update_refuses_labels_without_a_description():
    frames, descriptions, C, params, _, ref = _case("missed_class")
    ap = _new(C, params, groups=["weather"])
    out, labels = _batch([s for _, s in frames], descriptions)
    del labels[2]["description"]
    with pytest.raises(ValueError, match=r"labels\[2\]\['description'\]"):
        ap.update(out, labels, 5)
    assert ap.state()["frames"].shape[0] == 0                   # nothing was launched


def test_more_than_64_frames_in_one_update_are_split():
    frames, descriptions, C, params, _, ref = _case("missed_class")
    reps = 23                                                   # 69 frames in one update
    many = [(200 + i, frames[i % 3][1]) for i in range(3 * reps)]
    desc = [descriptions[i % 3] for i in range(3 * reps)]
    ap = _new(C, params, groups=["weather"])
    out, labels = _batch([s for _, s in many], desc)
    ap.update(out, labels, 200)
    res = ap.compute()
    fog, rain = res["group_names"].index("weather=fog"), res["group_names"].index("weather=rain")
    assert res["group_nframes"].tolist()[:1] == [69.0] and res["group_nframes"][fog] == reps and res["group_nframes"][rain] == 2 * reps
    assert res["group_npos"][fog].tolist() == (ref["npos"][ref["names"].index("weather=fog")] * reps).tolist()


# ------------------------------------------------------------------------------------------------- the public interface
class _Stub(torch.nn.Module):
    """A 'model' that returns precomputed head outputs: data['idx'] selects the frames of the batch."""

    def __init__(self, frames):
        super().__init__()
        self.out, _ = _batch([s for _, s in frames])
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward(self, data):
        return {k: v[data["idx"]] for k, v in self.out.items()}


class _StubLoss(torch.nn.Module):
    def forward(self, output, labels):
        loss = (output["center"] ** 2).mean()
        return loss, {"center": loss}


def _loader(frames, descriptions, bs):
    batches = []
    for i in range(0, len(frames), bs):
        chunk = frames[i:i + bs]
        _, labels = _batch([s for _, s in chunk], descriptions[i:i + bs], "host_f32")      # as the dataset delivers them
        batches.append(({"idx": torch.arange(i, i + len(chunk))}, labels))
    return batches


class _Writer:
    def __init__(self):
        self.tags = {}

    def add_scalar(self, tag, value, step):
        self.tags[tag] = (value, step)


def _record_calls(monkeypatch):
    from dpft_amd.hip.lib import lib
    calls, real = [], lib.call

    def call(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(lib, "call", call)
    return calls


def _plain_keys(ref, C):
    names = [f"{kind}@{thr:g}" for kind, thr in ref["combos"]]
    return {f"mAP_{n}" for n in names} | {f"AP_{n}/{c}" for n in names for c in range(1, C)} | {f"npos/{c}" for c in range(1, C)} | \
        {"dropped_nan"}


def _group_keys(ref, C):
    names = [f"{kind}@{thr:g}" for kind, thr in ref["combos"]]
    keys = {"bad_description"}
    for g in ref["names"][1:]:
        keys |= {f"mAP_{n}/{g}" for n in names} | {f"AP_{n}/{c}/{g}" for n in names for c in range(1, C)}
        keys |= {f"npos/{c}/{g}" for c in range(1, C)} | {f"nframes/{g}"}
    return keys


def _check_scalars(got, ref, C):
    for g, name in enumerate(ref["names"]):
        tail = "" if g == 0 else "/" + name
        for k, (kind, thr) in enumerate(ref["combos"]):
            assert _same(got[f"mAP_{kind}@{thr:g}{tail}"], ref["mAP"][g, k], AP_TOL), (name, kind, thr)
            for c in range(1, C):
                assert _same(got[f"AP_{kind}@{thr:g}/{c}{tail}"], ref["ap"][g, c - 1, k], AP_TOL)
        if g:
            assert got[f"nframes/{name}"] == ref["nframes"][g]
    assert got["bad_description"] == ref["bad_description"]


@pytest.mark.parametrize("groups", [None, ["weather"]])
def test_evaluate_one_epoch_returns_and_logs_the_group_tables_only_with_groups(monkeypatch, groups):
    from dpft_amd.configs import load_config
    from dpft_amd.evaluation import DataParallelEvaluator
    frames, descriptions, C, params, ref = G.stream_case()
    ref = ref if groups is None else G.run(frames, descriptions, C, groups, **params)
    cfg = copy.deepcopy(load_config("kradar"))
    cfg["model"]["head"]["num_classes"] = C
    cfg["computing"] = dict(cfg.get("computing", {}), device=DEV)
    cfg["evaluate"]["dataset_ap"] = {"iou": [0.3, 0.5, 0.7], "recall_points": 40, **({} if groups is None else {"groups": groups})}
    ev = DataParallelEvaluator.from_config(cfg)
    ev.eval_fn, ev.export_fn, ev.logging = None, None, "epoch"
    calls, w = _record_calls(monkeypatch), _Writer()
    got = ev.evaluate_one_epoch(2, _Stub(frames).to(DEV), _loader(frames, descriptions, 3), w, None, shard_start=frames[0][0])
    mine = [c for c in calls if "dataset_ap" in c]
    if groups is None:
        assert set(got) == _plain_keys(ref, C) and set(w.tags) == {f"test/{k}" for k in got}
        assert mine == ["dpft_dataset_ap_update_f32"] * 11 + ["dpft_dataset_ap_finalize_f64"]
        return
    assert set(got) == _plain_keys(ref, C) | _group_keys(ref, C) and set(w.tags) == {f"test/{k}" for k in got}
    assert mine == ["dpft_dataset_ap_update_groups_f32"] * 11 + ["dpft_dataset_ap_finalize_groups_f64"]
    _check_scalars(got, ref, C)
    assert w.tags["test/mAP_3d@0.5/weather=fog"] == (got["mAP_3d@0.5/weather=fog"], 2)


@pytest.mark.parametrize("groups", [None, True])
def test_trainer_validation_returns_and_logs_the_group_tables_only_with_groups(monkeypatch, groups):
    from dpft_amd.configs import load_config
    from dpft_amd.training.trainer import DataParallelTrainer
    frames, descriptions, C, params, ref = G.stream_case()
    cfg = copy.deepcopy(load_config("kradar"))
    cfg["train"]["optimizer"] = {"name": "AdamW", "lr": 1e-2}
    cfg["model"]["head"]["num_classes"] = C
    cfg["evaluate"] = {"dataset_ap": {"iou": [0.3, 0.5, 0.7], "recall_points": 40, **({} if groups is None else {"groups": groups})}}
    tr = DataParallelTrainer(_Stub(frames), cfg, torch.device(DEV))
    tr.loss_fn = _StubLoss()
    calls, w = _record_calls(monkeypatch), _Writer()
    res = tr.validate_one_epoch(1, _loader(frames, descriptions, 5), w)
    mine = [c for c in calls if "dataset_ap" in c]
    base = {"loss", "loss_center"} | _plain_keys(ref, C)
    if groups is None:
        assert set(res) == base and set(w.tags) == {f"val/{k}" for k in base}
        assert mine == ["dpft_dataset_ap_update_f32"] * 7 + ["dpft_dataset_ap_finalize_f64"]
        return
    assert set(res) == base | _group_keys(ref, C) and set(w.tags) == {f"val/{k}" for k in res}
    assert mine == ["dpft_dataset_ap_update_groups_f32"] * 7 + ["dpft_dataset_ap_finalize_groups_f64"]
    _check_scalars(res, ref, C)      # frames are numbered rank * 2^24 + local index: the same order as the reference's
    assert w.tags["val/nframes/time=night"] == (16.0, 1)
