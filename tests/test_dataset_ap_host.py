"""Host side of the split-level AP: config parsing, refusal of CPU tensors, and the C-ABI entry points' argument checks (all of
them happen before any launch, so none of this needs a GPU)."""
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
    from dpft_amd.evaluation.dataset_ap import DEFAULT_ROI, DatasetAP
    assert DatasetAP.from_config(_config(None)) is None
    assert DatasetAP.from_config(_config(False)) is None
    ap = DatasetAP.from_config(_config(True))
    assert ap.num_classes == 2 and ap.iou == [0.3, 0.5, 0.7] and ap.kinds == ["bev", "3d"] and ap.recall_points == 40
    assert ap.min_score == 0.0 and ap.roi == DEFAULT_ROI and len(ap.combinations) == 6
    assert ap.combinations[0] == ("bev", 0.3) and ap.combinations[3] == ("3d", 0.3)      # kinds outermost
    ap = DatasetAP.from_config(_config({"iou": [0.5], "kinds": ["3d"], "recall_points": 11, "min_score": 0.25, "roi": None}))
    assert ap.combinations == [("3d", 0.5)] and ap.recall_points == 11 and ap.min_score == 0.25 and ap.roi is None
    assert ap.key("3d", 0.5) == "3d@0.5"
    # nothing accumulated: NaN table, no library call
    res = ap.compute()
    assert res["mAP_3d@0.5"] != res["mAP_3d@0.5"] and res["npos/1"] == 0.0 and res["dropped_nan"] == 0.0
    assert set(ap.scalars()) == {"AP_3d@0.5/1", "mAP_3d@0.5", "npos/1", "dropped_nan"}


@pytest.mark.parametrize("spec, word", [
    ({"iou": [0.0]}, "iou"), ({"iou": [1.0]}, "iou"), ({"iou": [0.5, -0.1]}, "iou"), ({"iou": []}, "iou"), ({"iou": ["a"]}, "iou"),
    ({"recall_points": 1}, "recall_points"), ({"recall_points": 102}, "recall_points"), ({"recall_points": 40.0}, "recall_points"),
    ({"iou": [0.1, 0.2, 0.3, 0.4, 0.5]}, "combinations"),                     # 2 kinds x 5 = 10 > 8
    ({"kinds": ["bev", "bird"]}, "kinds"), ({"kinds": []}, "kinds"), ({"kinds": ["bev", "bev"]}, "kinds"),
    ({"roi": [0, 1, 2, 3, 4]}, "roi"), ({"roi": [0, 1, 2, 3, 4, float("inf")]}, "roi"), ({"roi": [0, 1, 2, 3, 4, float("nan")]}, "roi"),
    ({"roi": "all"}, "roi"), ({"min_score": "x"}, "min_score"), ({"threshold": 0.5}, "threshold"), ("yes", "dataset_ap"),
])
def test_from_config_names_the_bad_key(spec, word):
    from dpft_amd.evaluation.dataset_ap import DatasetAP
    with pytest.raises(ValueError, match=word):
        DatasetAP.from_config(_config(spec))


def test_evaluator_and_trainer_are_inert_without_the_key():
    from dpft_amd.evaluation import DataParallelEvaluator
    ev = DataParallelEvaluator(device=torch.device("cpu"))
    assert ev.dataset_ap is None
    ev = DataParallelEvaluator.from_config({**_config(None), "computing": {"device": "cpu"}})
    assert ev.dataset_ap is None
    ev = DataParallelEvaluator.from_config({**_config({"iou": [0.5]}), "computing": {"device": "cpu"}})
    assert ev.dataset_ap is not None and len(ev.dataset_ap.combinations) == 2


def test_cpu_tensors_are_refused():
    from dpft_amd.evaluation.dataset_ap import DatasetAP
    from dpft_amd.hip.lib import HipLibraryError
    ap = DatasetAP(3)
    out = {"class": torch.zeros(1, 4, 3), "center": torch.zeros(1, 4, 3), "size": torch.ones(1, 4, 3), "angle": torch.zeros(1, 4, 2)}
    lab = [{"gt_center": torch.zeros(1, 3), "gt_size": torch.ones(1, 3), "gt_angle": torch.zeros(1, 2), "gt_class": torch.zeros(1, 3)}]
    with pytest.raises(HipLibraryError, match="device tensors"):
        ap.update(out, lab, 0)


def _update_args(**over):
    """A call of dpft_dataset_ap_update_f32 with valid sizes and dangling (never dereferenced) non-null pointers."""
    p = C.c_void_p(4096)
    a = dict(cls=p, center=p, size=p, angle=p, gt_box=p, gt_id=p, counts=p, thr=(C.c_double * 8)(*[0.5] * 8),
             kinds=(C.c_int32 * 8)(*[0] * 8), K=1, roi=None, min_score=0.0, scratch=p, records=p, capacity=1 << 20, reserved=0,
             counters=p, first_frame=0, B=2, N=400, Mmax=30, Cn=8, stream=None)
    a.update(over)
    return [a[k] for k in ("cls", "center", "size", "angle", "gt_box", "gt_id", "counts", "thr", "kinds", "K", "roi", "min_score",
                           "scratch", "records", "capacity", "reserved", "counters", "first_frame", "B", "N", "Mmax", "Cn", "stream")]


@pytest.mark.parametrize("over, word", [
    (dict(cls=None), "null"), (dict(gt_id=None), "null"), (dict(scratch=None), "null"), (dict(records=None), "null"),
    (dict(counters=None), "null"), (dict(thr=None), "null"), (dict(kinds=None), "null"),
    (dict(N=1025), "sizes out of range"), (dict(Mmax=257), "sizes out of range"), (dict(Cn=17), "sizes out of range"),
    (dict(Cn=1), "sizes out of range"), (dict(B=0), "sizes out of range"),
    (dict(K=0), "combinations"), (dict(K=9), "combinations"),
    (dict(capacity=799), "record store too small"), (dict(capacity=1000, reserved=201), "record store too small"),
    (dict(thr=(C.c_double * 8)(*[1.0] * 8)), "threshold inside"), (dict(kinds=(C.c_int32 * 8)(*[2] * 8)), "threshold inside"),
    (dict(roi=(C.c_float * 6)(0, 1, 2, 3, 4, float("inf"))), "not finite"),
    (dict(records=C.c_void_p(4100)), "alignment"),
])
def test_update_entry_refuses_before_any_launch(over, word):
    from dpft_amd.hip.lib import lib
    rc = lib.load().dpft_dataset_ap_update_f32(*_update_args(**over))
    assert rc != 0 and word in lib.dpft_last_error().decode()


def test_finalize_and_scratch_entries_refuse_before_any_launch():
    from dpft_amd.hip.lib import lib
    dll, p = lib.load(), C.c_void_p(4096)
    good = dict(rec=p, n=10, start=p, counters=p, Cn=8, K=6, R=40, ap=p, npos=p, tp=p, stream=None)
    order = ("rec", "n", "start", "counters", "Cn", "K", "R", "ap", "npos", "tp", "stream")
    for over, word in [(dict(rec=None), "null"), (dict(start=None), "null"), (dict(counters=None), "null"), (dict(ap=None), "null"),
                       (dict(npos=None), "null"), (dict(tp=None), "null"), (dict(R=1), "sizes out of range"),
                       (dict(R=102), "sizes out of range"), (dict(K=0), "sizes out of range"), (dict(K=9), "sizes out of range"),
                       (dict(Cn=17), "sizes out of range"), (dict(Cn=1), "sizes out of range"), (dict(n=-1), "sizes out of range")]:
        a = dict(good, **over)
        rc = dll.dpft_dataset_ap_finalize_f64(*[a[k] for k in order])
        assert rc != 0 and word in lib.dpft_last_error().decode(), over
    assert dll.dpft_dataset_ap_scratch_bytes(4, 400, 30) == 4 * 400 * 30 * 16
    assert dll.dpft_dataset_ap_scratch_bytes(3, 1024, 256) == 3 * 1024 * 256 * 16
    for bad in [(1, 1025, 1), (1, 1, 257), (0, 1, 1), (1, 0, 1), (1, 1, 0)]:
        assert dll.dpft_dataset_ap_scratch_bytes(*bad) == -1 and "out of range" in lib.dpft_last_error().decode()


def _gather_worker(rank, world, port, q):
    import torch.distributed as dist
    from dpft_amd.evaluation.dataset_ap import gather_state
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    n = (5, 0, 3)[rank]                                       # unequal counts, one rank without records
    records = (torch.arange(n * 4, dtype=torch.int32).reshape(n, 4) + 1000 * rank)
    counters = torch.zeros(32, dtype=torch.int64)
    counters[0], counters[1], counters[16 + 1], counters[16 + 2] = n, rank, 10 * rank + 1, 7
    out = gather_state({"records": records, "counters": counters})
    q.put((rank, out["records"].numpy(), out["counters"].numpy()))
    dist.destroy_process_group()


def test_gather_state_gives_every_rank_all_records_and_the_summed_counters():
    """The multi-rank collective on raw state tensors, three gloo ranks on the CPU."""
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
    res = {r: (rec, cnt) for r, rec, cnt in (q.get(timeout=120) for _ in range(world))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = np.concatenate([np.arange(20).reshape(5, 4), np.arange(12).reshape(3, 4) + 2000]).astype(np.int32)
    for r in range(world):
        rec, cnt = res[r]
        assert np.array_equal(rec, want)
        assert cnt[0] == 8 and cnt[1] == 3 and cnt[17] == 33 and cnt[18] == 21 and cnt.sum() == 8 + 3 + 33 + 21
