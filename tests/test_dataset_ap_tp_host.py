"""Host side of the true-positive errors of the split-level AP (evaluate.dataset_ap.tp_errors): config parsing and its refusals,
state / load_state / merge on empty accumulators, gather_state over gloo ranks, the entries' argument checks (before any launch)
and what stays exactly as it is without the key.  No GPU."""
import copy
import ctypes as C
import os
import socket

import pytest
import torch


def _config(spec):
    from dpft_amd.configs import load_config
    cfg = copy.deepcopy(load_config("kradar"))
    if spec is not None:
        cfg["evaluate"]["dataset_ap"] = spec
    return cfg


def test_from_config_defaults_and_overrides():
    from dpft_amd.evaluation.dataset_ap import DatasetAP
    ap = DatasetAP.from_config(_config({"tp_errors": True}))
    assert ap.tp == {"at": ("bev", 0.3), "k": 0, "min_recall": 0.1, "i_min": 4, "angle_period": "2pi"}
    ap = DatasetAP.from_config(_config({"iou": [0.7, 0.5], "kinds": ["3d", "bev"], "tp_errors": {}}))
    assert ap.tp["at"] == ("3d", 0.5) and ap.tp["k"] == 1               # the first kind, the smallest threshold
    ap = DatasetAP.from_config(_config({"tp_errors": {"at": ["3d", 0.7], "min_recall": 0, "angle_period": "pi"},
                                        "recall_points": 101}))
    assert ap.tp == {"at": ("3d", 0.7), "k": 5, "min_recall": 0.0, "i_min": 1, "angle_period": "pi"}
    for m, R, want in ((0.1, 40, 4), (0.1, 101, 11), (0.3, 40, 12), (0.7, 40, 28), (1, 40, 40), (1.0, 2, 2), (0.29, 100, 29)):
        assert DatasetAP(2, recall_points=R, tp_errors={"min_recall": m}).tp["i_min"] == want, (m, R)
    for off in (None, False):
        assert DatasetAP.from_config(_config({"tp_errors": off})).tp is None
    assert DatasetAP.from_config(_config(True)).tp is None


@pytest.mark.parametrize("spec, word", [
    ({"at": ["bev", 0.4]}, "'at'"), ({"at": ["bird", 0.3]}, "'at'"), ({"at": "bev"}, "'at'"), ({"at": ["bev"]}, "'at'"),
    ({"at": [0.3, "bev"]}, "'at'"), ({"at": ["bev", True]}, "'at'"),
    ({"min_recall": -0.01}, "min_recall"), ({"min_recall": 1.01}, "min_recall"), ({"min_recall": "0.1"}, "min_recall"),
    ({"min_recall": None}, "min_recall"), ({"min_recall": float("nan")}, "min_recall"), ({"min_recall": True}, "min_recall"),
    ({"angle_period": "tau"}, "angle_period"), ({"angle_period": 3.14}, "angle_period"), ({"angle_period": None}, "angle_period"),
    ({"period": "pi"}, "period"), ("yes", "tp_errors"), (1, "tp_errors"),
])
def test_from_config_names_the_bad_key(spec, word):
    from dpft_amd.evaluation.dataset_ap import DatasetAP
    with pytest.raises(ValueError, match=word):
        DatasetAP.from_config(_config({"tp_errors": spec}))
    with pytest.raises(ValueError, match=word):
        DatasetAP(2, tp_errors=spec)


def test_at_must_be_a_configured_combination_and_unknown_keys_stay_refused():
    from dpft_amd.evaluation.dataset_ap import DatasetAP
    with pytest.raises(ValueError, match="'at'"):
        DatasetAP.from_config(_config({"kinds": ["3d"], "tp_errors": {"at": ["bev", 0.3]}}))
    with pytest.raises(ValueError, match="tp_error"):
        DatasetAP.from_config(_config({"tp_error": True}))
    with pytest.raises(ValueError, match="threshold"):
        DatasetAP.from_config(_config({"threshold": 0.5, "tp_errors": True}))


def _keys(ap):
    names = [f"{kind}@{thr:g}" for kind, thr in ap.combinations]
    Cn = ap.num_classes
    return {f"mAP_{n}" for n in names} | {f"AP_{n}/{c}" for n in names for c in range(1, Cn)} | {f"npos/{c}" for c in range(1, Cn)} | \
        {"dropped_nan"}


def _tp_keys(Cn, tail=""):
    return {f"{e}/{c}{tail}" for e in ("ATE", "AZE", "ASE", "AOE") for c in range(1, Cn)} | \
        {f"m{e}{tail}" for e in ("ATE", "AZE", "ASE", "AOE")} | {f"tp_points/{c}{tail}" for c in range(1, Cn)}


def test_nothing_accumulated_gives_nan_and_without_the_key_nothing_is_new():
    from dpft_amd.evaluation.dataset_ap import DatasetAP
    plain, tp = DatasetAP(3), DatasetAP(3, tp_errors=True)
    assert set(plain.state()) == {"records", "counters"} and set(plain.scalars()) == _keys(plain)
    assert set(plain.compute()) == _keys(plain) | {"ap", "npos", "tp"}
    st = tp.state()
    assert set(st) == {"records", "counters", "tp_errors"} and st["tp_errors"].shape == (0, 4) and st["tp_errors"].dtype == torch.int64
    res = tp.compute()
    assert set(tp.scalars()) == _keys(tp) | _tp_keys(3) | {"tp_saturated"}
    assert set(res) == set(tp.scalars()) | {"ap", "npos", "tp", "tp_err", "tp_points"}
    assert res["tp_err"].shape == (2, 4) and res["tp_err"].dtype == torch.float64 and torch.isnan(res["tp_err"]).all()
    assert res["tp_points"].tolist() == [0.0, 0.0] and res["tp_saturated"] == 0.0 and res["mATE"] != res["mATE"]
    assert res["AOE/2"] != res["AOE/2"] and res["tp_points/1"] == 0.0
    # with groups: the same keys per group, with the AP keys' suffix
    both = DatasetAP(3, tp_errors=True, groups=["time"])
    res = both.compute()
    assert set(both.state()) == {"records", "counters", "frames", "tp_errors"}
    assert _tp_keys(3) | _tp_keys(3, "/time=day") | _tp_keys(3, "/time=night") | {"tp_saturated"} <= set(both.scalars())
    assert not any(k.startswith("ATE") and k.endswith("/all") for k in res)
    assert res["group_tp_err"].shape == (3, 2, 4) and res["group_tp_points"].shape == (3, 2) and torch.isnan(res["group_tp_err"]).all()
    grouped = DatasetAP(3, groups=["time"])
    assert not any(k.startswith(("ATE", "mATE", "tp_", "group_tp_")) for k in grouped.compute())


def test_state_load_state_and_merge_on_the_host():
    from dpft_amd.evaluation.dataset_ap import DatasetAP
    a, b = DatasetAP(3, tp_errors=True), DatasetAP(3, tp_errors=True)
    a.merge(b)                                                              # two empty accumulators
    assert a.state()["tp_errors"].shape == (0, 4)
    a.load_state(b.state())
    with pytest.raises(ValueError, match="tp_errors"):
        a.load_state({k: v for k, v in b.state().items() if k != "tp_errors"})
    with pytest.raises(ValueError, match="tp_errors"):
        a.load_state(dict(b.state(), tp_errors=torch.zeros((0, 4), dtype=torch.int32)))
    with pytest.raises(ValueError, match="tp_errors"):
        a.load_state(dict(b.state(), tp_errors=torch.zeros((2, 4), dtype=torch.int64)))      # not parallel to the records
    DatasetAP(3).load_state(b.state())                                      # without the key the extra tensor is not looked at
    for other in (DatasetAP(3), DatasetAP(3, tp_errors={"min_recall": 0.2}), DatasetAP(3, tp_errors={"angle_period": "pi"}),
                  DatasetAP(3, tp_errors={"at": ["3d", 0.3]})):
        with pytest.raises(ValueError, match="differ"):
            a.merge(other)
        with pytest.raises(ValueError, match="differ"):
            other.merge(a)
    a.reset()
    assert a._tp_rows is None and a.capacity == 0


def _update_args(**over):
    """A call of dpft_dataset_ap_update_tp_f32 with valid sizes and dangling (never dereferenced) non-null pointers."""
    p = C.c_void_p(4096)
    a = dict(cls=p, center=p, size=p, angle=p, gt_box=p, gt_id=p, counts=p, thr=(C.c_double * 8)(*[0.5] * 8),
             kinds=(C.c_int32 * 8)(*[0] * 8), K=2, roi=None, min_score=0.0, scratch=p, records=p, capacity=1 << 20, reserved=0,
             counters=p, first_frame=0, B=2, N=400, Mmax=30, Cn=8, rows=p, ref_k=1, fold=0, stream=None)
    a.update(over)
    return [a[k] for k in ("cls", "center", "size", "angle", "gt_box", "gt_id", "counts", "thr", "kinds", "K", "roi", "min_score",
                           "scratch", "records", "capacity", "reserved", "counters", "first_frame", "B", "N", "Mmax", "Cn", "rows",
                           "ref_k", "fold", "stream")]


@pytest.mark.parametrize("over, word", [
    (dict(rows=None), "null"), (dict(cls=None), "null"), (dict(records=None), "null"), (dict(rows=C.c_void_p(4104)), "alignment"),
    (dict(ref_k=2), "reference combination"), (dict(ref_k=-1), "reference combination"), (dict(fold=2), "fold_pi"),
    (dict(N=1025), "sizes out of range"), (dict(K=9), "combinations"), (dict(K=9, ref_k=9), "reference combination"),
    (dict(capacity=799), "record store too small"),
])
def test_update_tp_entry_refuses_before_any_launch(over, word):
    from dpft_amd.hip.lib import lib
    rc = lib.load().dpft_dataset_ap_update_tp_f32(*_update_args(**over))
    assert rc != 0 and word in lib.dpft_last_error().decode(), lib.dpft_last_error()


def test_update_groups_tp_and_finalize_tp_entries_refuse_before_any_launch():
    from dpft_amd.hip.lib import lib
    dll, p = lib.load(), C.c_void_p(4096)
    base = _update_args()
    groups = [p, p, p, p, p, p, 0, p, 8, 0]      # descriptions, axis tables, n_axes, frames, frame capacity, frames before
    assert len(base) == 26
    for over, word in [(dict(rows=None), "null"), (dict(ref_k=2), "reference combination"), (dict(fold=-1), "fold_pi")]:
        a = _update_args(**over)      # (the true-positive arguments are checked first: the dangling host pointers are never read)
        rc = dll.dpft_dataset_ap_update_groups_tp_f32(*a[:22], *groups, *a[22:])
        assert rc != 0 and word in lib.dpft_last_error().decode(), over
    good = dict(rec=p, rows=p, n=10, start=p, counters=p, Cn=8, k=0, R=40, i_min=4, err=p, points=p, stream=None)
    order = ("rec", "rows", "n", "start", "counters", "Cn", "k", "R", "i_min", "err", "points", "stream")
    for over, word in [(dict(rec=None), "null"), (dict(rows=None), "null"), (dict(start=None), "null"), (dict(counters=None), "null"),
                       (dict(err=None), "null"), (dict(points=None), "null"), (dict(R=1), "sizes out of range"),
                       (dict(R=102), "sizes out of range"), (dict(k=8), "sizes out of range"), (dict(k=-1), "sizes out of range"),
                       (dict(Cn=17), "sizes out of range"), (dict(n=-1), "sizes out of range"), (dict(i_min=0), "first recall point"),
                       (dict(i_min=41), "first recall point"), (dict(rows=C.c_void_p(4104)), "alignment")]:
        a = dict(good, **over)
        rc = dll.dpft_dataset_ap_finalize_tp_f64(*[a[k] for k in order])
        assert rc != 0 and word in lib.dpft_last_error().decode(), over
    good = dict(rec=p, rows=p, groups=p, n=10, start=p, npos=p, G=3, Cn=8, k=0, R=40, i_min=4, err=p, points=p, stream=None)
    order = ("rec", "rows", "groups", "n", "start", "npos", "G", "Cn", "k", "R", "i_min", "err", "points", "stream")
    for over, word in [(dict(groups=None), "null"), (dict(npos=None), "null"), (dict(rec=None), "null"), (dict(G=0), "1..32 groups"),
                       (dict(G=33), "1..32 groups"), (dict(i_min=41), "first recall point"), (dict(k=8), "sizes out of range")]:
        a = dict(good, **over)
        rc = dll.dpft_dataset_ap_finalize_tp_groups_f64(*[a[k] for k in order])
        assert rc != 0 and word in lib.dpft_last_error().decode(), over


def _gather_worker(rank, world, port, q):
    import torch.distributed as dist
    from dpft_amd.evaluation.dataset_ap import gather_state
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    n = (5, 0, 3)[rank]                                       # unequal counts, one rank without records
    records = (torch.arange(n * 4, dtype=torch.int32).reshape(n, 4) + 1000 * rank)
    rows = (torch.arange(n * 4, dtype=torch.int64).reshape(n, 4) + (1 << 40) * (rank + 1))
    counters = torch.zeros(32, dtype=torch.int64)
    counters[0], counters[3], counters[16 + 1] = n, rank + 1, 7
    out = gather_state({"records": records, "counters": counters, "tp_errors": rows})
    plain = gather_state({"records": records, "counters": counters})
    q.put((rank, out["records"].numpy(), out["counters"].numpy(), out["tp_errors"].numpy(), sorted(plain)))
    dist.destroy_process_group()


def test_gather_state_gathers_the_error_rows_like_the_records():
    """Three gloo ranks on the CPU: every rank ends up with all ranks' rows in rank order, parallel to the records."""
    import numpy as np
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {r: rest for r, *rest in (q.get(timeout=120) for _ in range(world))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want_rec = np.concatenate([np.arange(20).reshape(5, 4), np.arange(12).reshape(3, 4) + 2000]).astype(np.int32)
    want_rows = np.concatenate([np.arange(20).reshape(5, 4) + (1 << 40), np.arange(12).reshape(3, 4) + 3 * (1 << 40)]).astype(np.int64)
    for r in range(world):
        rec, cnt, rows, plain_keys = res[r]
        assert np.array_equal(rec, want_rec) and rows.dtype == np.int64 and np.array_equal(rows, want_rows)
        assert cnt[0] == 8 and cnt[3] == 6 and cnt[17] == 21
        assert plain_keys == ["counters", "records"]          # without the key's tensor nothing new is gathered
