"""Cost of the split-level AP (evaluate.dataset_ap), between device events, in one run:

1. ``DatasetAP.update`` at B = 4, N = 400, C = 8, about 30 targets per sample, K = 6 combinations, beside ``Metric.forward`` on the
   same tensors (both include their ``pack_targets`` launch and host work); and the two update launches alone
   (``dpft_dataset_ap_update_f32`` with pre-packed targets) beside ``dpft_detection_metrics_f32`` alone.
2. ``DatasetAP.compute()`` on about 2 * 10^5 records (wall clock: it ends with a read-back), split into its sort (torch) and the
   finalize launch.

With ``--groups`` the groups leg instead (evaluate.dataset_ap.groups, all three axes = 19 groups), every figure beside the
ungrouped one of the same process:

3. ``DatasetAP.update`` with and without groups on the same tensors (descriptions on the device, and on the host).
4. ``DatasetAP.compute()`` on about 2 * 10^5 records with 19 groups beside the ungrouped ``compute()`` on the same records, and
   the two finalize entries alone between device events.

With ``--tp-errors`` the true-positive errors' leg instead (evaluate.dataset_ap.tp_errors), every figure beside the run without the
key in the same process:

5. ``DatasetAP.update`` with and without the key on the same tensors, measured twice each (a, b, a, b): the two figures of one
   side show the run-to-run spread that a difference has to exceed; and the update entries alone on pre-packed targets.
6. ``DatasetAP.compute()`` on about 2 * 10^5 records with and without the key, and the two finalize entries alone.

With ``--kitti`` the KITTI-protocol table's leg instead (evaluate.dataset_ap.kitti), every figure beside the run without the key
in the same process:

7. ``DatasetAP.update`` with and without the key on the same tensors, measured twice each (a, b, a, b), and the update entries
   alone on pre-packed targets.
8. ``DatasetAP.compute()`` on about 2 * 10^5 records with and without the key, and the two finalize entries alone.

Prints JSON lines and writes them to ``--out`` (default profiles/dataset_ap.txt, with ``--groups`` profiles/dataset_ap_groups.txt,
with ``--tp-errors`` profiles/dataset_ap_tp.txt, with ``--kitti`` profiles/dataset_ap_kitti.txt).
Usage: python tools/dataset_ap_cost.py [--groups | --tp-errors | --kitti] [--reps 200] [--records 200000] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--records", type=int, default=200000)
    p.add_argument("--groups", action="store_true", help="the groups leg (3., 4.) instead of 1. and 2.")
    p.add_argument("--tp-errors", action="store_true", help="the true-positive errors' leg (5., 6.) instead of 1. and 2.")
    p.add_argument("--kitti", action="store_true", help="the KITTI-protocol table's leg (7., 8.) instead of 1. and 2.")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.groups + args.tp_errors + args.kitti > 1:
        p.error("--groups, --tp-errors and --kitti are separate legs")
    if args.out is None:
        name = "dataset_ap_groups.txt" if args.groups else "dataset_ap_tp.txt" if args.tp_errors else \
            "dataset_ap_kitti.txt" if args.kitti else "dataset_ap.txt"
        args.out = os.path.join(ROOT, "profiles", name)
    import numpy as np
    import torch
    import dataset_ap_ref as R                                  # the tests' seeded sample builder
    from dpft_amd.evaluation.dataset_ap import KINDS, DatasetAP
    from dpft_amd.evaluation.metric import Metric
    from dpft_amd.hip.lib import lib, stream
    from dpft_amd.training.loss import pack_targets

    assert torch.cuda.is_available(), "dataset_ap_cost.py measures on the GPU; there is nothing to measure without one"
    dev = torch.device("cuda", 0)
    B, N, Cn = 4, 400, 8
    rng = np.random.default_rng(0)
    samples = [R.random_sample(rng, N, int(m), Cn) for m in rng.integers(26, 35, B)]
    out = {k: torch.from_numpy(np.stack([s[src] for s in samples])).to(dev)
           for k, src in (("class", "cls"), ("center", "center"), ("size", "size"), ("angle", "angle"))}
    labels = [{k: torch.from_numpy(s[k]).to(dev) for k in ("gt_center", "gt_size", "gt_angle", "gt_class")} for s in samples]
    ap = DatasetAP(Cn, initial_capacity=1 << 22)                # (no growth inside the timed region)
    metric = Metric(metrics={"mAP": "mAP3D", "mGIoU": "mGIoU3D"})
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    def timed(fn):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
        return {"median_us": round(statistics.median(t), 1), "min_us": round(t[0], 1), "p90_us": round(t[int(0.9 * len(t))], 1)}

    if args.groups:
        groups_leg(args, torch, DatasetAP, lib, stream, dev, out, labels, B, N, Cn, timed, emit)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return

    if args.tp_errors:
        tp_leg(args, torch, DatasetAP, KINDS, pack_targets, lib, stream, dev, out, labels, B, N, Cn, timed, emit)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return

    if args.kitti:
        kitti_leg(args, torch, DatasetAP, KINDS, pack_targets, lib, stream, dev, out, labels, B, N, Cn, timed, emit)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return

    frame = [0]

    def update():
        ap.update(out, labels, frame[0])
        frame[0] += B

    # the entries alone, on pre-packed targets
    counts = [int(l["gt_class"].shape[0]) for l in labels]
    gt_box, gt_onehot, gt_id, counts_t, Mmax = pack_targets(labels, counts, Cn, dev)
    K = len(ap.combinations)
    thr = (C.c_double * K)(*[t for _, t in ap.combinations])
    kinds = (C.c_int32 * K)(*[KINDS.index(k) for k, _ in ap.combinations])
    roi = (C.c_float * 6)(*ap.roi)
    scratch = torch.empty(int(lib.dpft_dataset_ap_scratch_bytes(B, N, Mmax)) // 8, dtype=torch.float64, device=dev)
    records = torch.empty((1 << 22, 4), dtype=torch.int32, device=dev)
    counters = torch.zeros(32, dtype=torch.int64, device=dev)
    reserved = [0]
    t4 = [out[k].contiguous() for k in ("class", "center", "size", "angle")]

    def update_alone():
        lib.call("dpft_dataset_ap_update_f32", *[t.data_ptr() for t in t4], gt_box.data_ptr(), gt_id.data_ptr(), counts_t.data_ptr(),
                 thr, kinds, K, roi, 0.0, scratch.data_ptr(), records.data_ptr(), records.shape[0], reserved[0], counters.data_ptr(),
                 0, B, N, Mmax, Cn, stream())
        reserved[0] += B * N

    mscratch = torch.empty((B, N, Mmax, 2), dtype=torch.float32, device=dev)
    mout = torch.empty((B, 2), dtype=torch.float32, device=dev)

    def metric_alone():
        lib.call("dpft_detection_metrics_f32", *[t.data_ptr() for t in t4], gt_box.data_ptr(), gt_onehot.data_ptr(),
                 counts_t.data_ptr(), 0.5, 101, mscratch.data_ptr(), mout.data_ptr(), B, N, Mmax, Cn, stream())

    update()
    n_det = int(ap.state()["counters"][0])
    emit({"what": "update beside Metric.forward, between device events", "device": torch.cuda.get_device_name(0), "B": B, "N": N,
          "C": Cn, "targets": counts, "K": K, "detections_per_update": n_det, "reps": args.reps,
          "DatasetAP.update": timed(update), "Metric.forward": timed(lambda: metric(out, labels)),
          "dpft_dataset_ap_update_f32 alone": timed(update_alone), "dpft_detection_metrics_f32 alone": timed(metric_alone)})

    # compute() on ~ --records records: the same batch under new frame numbers
    ap.reset()
    frame[0] = 0
    while ap._bound < args.records * N // max(n_det // B, 1):
        update()
    torch.cuda.synchronize()
    walls, parts = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        st = ap.state()
        t1 = time.perf_counter()
        DatasetAP.sort_records(st["records"])
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        res = ap.compute()
        t3 = time.perf_counter()
        walls.append((t3 - t2) * 1e3)
        parts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
    n = int(ap.state()["records"].shape[0])
    emit({"what": "compute() wall clock, ms (state read-back + sort + finalize launch + result read-back)", "records": n,
          "compute_ms_median": round(statistics.median(walls), 2), "compute_ms_min": round(min(walls), 2),
          "of_which_state_ms": round(statistics.median(a for a, _ in parts), 2),
          "of_which_sort_ms": round(statistics.median(b for _, b in parts), 2),
          "mAP_3d@0.5": res["mAP_3d@0.5"]})
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def groups_leg(args, torch, DatasetAP, lib, stream, dev, out, labels, B, N, Cn, timed, emit):
    """3. and 4. of the module docstring: a grouped and an ungrouped accumulator fed the same batches in the same process."""
    def described(where, first):
        return [dict(l, description=torch.tensor([(first + b) % 9, (first + b) % 2, (first + b) % 7], dtype=torch.float32).to(where))
                for b, l in enumerate(labels)]
    plain, grouped = DatasetAP(Cn, initial_capacity=1 << 22), DatasetAP(Cn, initial_capacity=1 << 22, groups=True,
                                                                         initial_frame_capacity=1 << 16)
    on_dev, on_host = described(dev, 0), described("cpu", 0)
    frame = {"plain": 0, "dev": 0, "host": 0}

    def update(ap, labs, key):
        def fn():
            ap.update(out, labs, frame[key])
            frame[key] += B
        return fn

    plain.update(out, labels, 0)
    n_det = int(plain.state()["counters"][0])
    plain.reset()
    t_plain = timed(update(plain, labels, "plain"))
    t_dev = timed(update(grouped, on_dev, "dev"))
    grouped.reset()
    t_host = timed(update(grouped, on_host, "host"))
    emit({"what": "update with and without groups, between device events", "device": torch.cuda.get_device_name(0), "B": B, "N": N,
          "C": Cn, "K": len(plain.combinations), "groups": len(grouped.group_names), "detections_per_update": n_det, "reps": args.reps,
          "DatasetAP.update without groups": t_plain, "DatasetAP.update with groups, descriptions on the device": t_dev,
          "DatasetAP.update with groups, descriptions on the host": t_host})

    # compute() on ~ --records records: the same batch under new frame numbers, the descriptions walking all 19 groups
    plain.reset()
    grouped.reset()
    first = 0
    while plain._bound < args.records * N // max(n_det // B, 1):
        plain.update(out, labels, first)
        grouped.update(out, described(dev, first), first)
        first += B
    torch.cuda.synchronize()
    walls = {"plain": [], "grouped": []}
    for _ in range(5):
        for key, ap in (("plain", plain), ("grouped", grouped)):
            t0 = time.perf_counter()
            res = ap.compute()
            walls[key].append((time.perf_counter() - t0) * 1e3)
    assert torch.equal(res["group_ap"][0].view(torch.int64), plain.compute()["ap"].view(torch.int64))

    # the finalize entries alone, on the sorted records
    st = grouped.state()
    rec = DatasetAP.sort_records(st["records"])
    n, F, G, K = int(rec.shape[0]), int(st["frames"].shape[0]), len(grouped.group_names), len(plain.combinations)
    cls_of = (rec[:, 2] >> 16) & 0xFF
    start = torch.searchsorted(cls_of.contiguous(), torch.arange(Cn + 1, dtype=cls_of.dtype, device=dev)).to(torch.int64)
    order = torch.sort(st["frames"][:, 0]).indices
    frame_of, mask_of = st["frames"][order, 0].contiguous(), st["frames"][order, 1]
    rec_groups = mask_of[torch.searchsorted(frame_of, rec[:, 1].contiguous())].contiguous()
    buf = torch.empty(G * (Cn - 1) * (2 * K + 1) + G + 1, dtype=torch.float64, device=dev)
    o = [0, G * (Cn - 1) * K, 2 * G * (Cn - 1) * K, 2 * G * (Cn - 1) * K + G * (Cn - 1), 2 * G * (Cn - 1) * K + G * (Cn - 1) + G]
    masks = (C.c_uint32 * 3)(0x6, 0xFF8, 0x7F000)

    def finalize_groups():
        lib.call("dpft_dataset_ap_finalize_groups_f64", rec.data_ptr(), rec_groups.data_ptr(), n, start.data_ptr(),
                 st["frames"].data_ptr(), F, masks, 3, G, Cn, K, 40, buf[o[0]:].data_ptr(), buf[o[2]:].data_ptr(),
                 buf[o[1]:].data_ptr(), buf[o[3]:].data_ptr(), buf[o[4]:].data_ptr(), stream())

    def finalize_plain():
        lib.call("dpft_dataset_ap_finalize_f64", rec.data_ptr(), n, start.data_ptr(), st["counters"].data_ptr(), Cn, K, 40,
                 buf[o[0]:].data_ptr(), buf[o[2]:].data_ptr(), buf[o[1]:].data_ptr(), stream())

    emit({"what": "compute() wall clock, ms, with 19 groups beside the ungrouped compute() on the same records", "records": n,
          "frames": F, "groups": G, "compute_ms_median without groups": round(statistics.median(walls["plain"]), 2),
          "compute_ms_median with groups": round(statistics.median(walls["grouped"]), 2),
          "compute_ms_min without groups": round(min(walls["plain"]), 2), "compute_ms_min with groups": round(min(walls["grouped"]), 2),
          "dpft_dataset_ap_finalize_f64 alone": timed(finalize_plain),
          "dpft_dataset_ap_finalize_groups_f64 alone (one workgroup per group, class, combination)": timed(finalize_groups),
          "mAP_3d@0.5/weather=fog": res["mAP_3d@0.5/weather=fog"]})


def tp_leg(args, torch, DatasetAP, KINDS, pack_targets, lib, stream, dev, out, labels, B, N, Cn, timed, emit):
    """5. and 6. of the module docstring: an accumulator with the key and one without, fed the same batches in the same process."""
    plain, tp = DatasetAP(Cn, initial_capacity=1 << 22), DatasetAP(Cn, initial_capacity=1 << 22, tp_errors=True)
    frame = {"plain": 0, "tp": 0}

    def update(ap, key):
        def fn():
            ap.update(out, labels, frame[key])
            frame[key] += B
        return fn

    plain.update(out, labels, 0)
    n_det = int(plain.state()["counters"][0])
    n_tp = int(((plain.state()["records"][:, 3] >> tp.tp["k"]) & 1).sum())
    plain.reset()
    t_plain, t_tp = [], []
    for _ in range(2):                                          # a, b, a, b: the spread of one side beside the difference
        t_plain.append(timed(update(plain, "plain")))
        t_tp.append(timed(update(tp, "tp")))

    # the entries alone, on pre-packed targets
    counts = [int(l["gt_class"].shape[0]) for l in labels]
    gt_box, _, gt_id, counts_t, Mmax = pack_targets(labels, counts, Cn, dev)
    K = len(plain.combinations)
    thr = (C.c_double * K)(*[t for _, t in plain.combinations])
    kinds = (C.c_int32 * K)(*[KINDS.index(k) for k, _ in plain.combinations])
    roi = (C.c_float * 6)(*plain.roi)
    scratch = torch.empty(int(lib.dpft_dataset_ap_scratch_bytes(B, N, Mmax)) // 8, dtype=torch.float64, device=dev)
    records = torch.empty((1 << 22, 4), dtype=torch.int32, device=dev)
    rows = torch.empty((1 << 22, 4), dtype=torch.int64, device=dev)
    counters = torch.zeros(32, dtype=torch.int64, device=dev)
    reserved = [0]
    t4 = [out[k].contiguous() for k in ("class", "center", "size", "angle")]

    def entry(name, *extra):
        def fn():
            if reserved[0] + B * N > records.shape[0]:
                reserved[0] = 0
                counters.zero_()
            lib.call(name, *[t.data_ptr() for t in t4], gt_box.data_ptr(), gt_id.data_ptr(), counts_t.data_ptr(), thr, kinds, K, roi,
                     0.0, scratch.data_ptr(), records.data_ptr(), records.shape[0], reserved[0], counters.data_ptr(), 0, B, N, Mmax,
                     Cn, *extra, stream())
            reserved[0] += B * N
        return fn

    e_plain, e_tp = [], []
    for _ in range(2):
        e_plain.append(timed(entry("dpft_dataset_ap_update_f32")))
        e_tp.append(timed(entry("dpft_dataset_ap_update_tp_f32", rows.data_ptr(), tp.tp["k"], 0)))
    emit({"what": "update with and without tp_errors, between device events, each side measured twice (a, b, a, b)",
          "device": torch.cuda.get_device_name(0), "B": B, "N": N, "C": Cn, "targets": counts, "K": K, "at": list(tp.tp["at"]),
          "detections_per_update": n_det, "tps_per_update": n_tp, "reps": args.reps,
          "DatasetAP.update without tp_errors": t_plain, "DatasetAP.update with tp_errors": t_tp,
          "dpft_dataset_ap_update_f32 alone": e_plain, "dpft_dataset_ap_update_tp_f32 alone": e_tp})

    # compute() on ~ --records records: the same batch under new frame numbers
    plain.reset()
    tp.reset()
    first = 0
    while plain._bound < args.records * N // max(n_det // B, 1):
        plain.update(out, labels, first)
        tp.update(out, labels, first)
        first += B
    torch.cuda.synchronize()
    walls = {"plain": [], "tp": []}
    for _ in range(5):
        for key, ap in (("plain", plain), ("tp", tp)):
            t0 = time.perf_counter()
            res = ap.compute()
            walls[key].append((time.perf_counter() - t0) * 1e3)
    assert torch.equal(res["ap"].view(torch.int64), plain.compute()["ap"].view(torch.int64))

    # the finalize entries alone, on the sorted records
    st = tp.state()
    perm = DatasetAP.sort_permutation(st["records"])
    rec, srows = st["records"][perm].contiguous(), st["tp_errors"][perm].contiguous()
    n = int(rec.shape[0])
    cls_of = (rec[:, 2] >> 16) & 0xFF
    start = torch.searchsorted(cls_of.contiguous(), torch.arange(Cn + 1, dtype=cls_of.dtype, device=dev)).to(torch.int64)
    buf = torch.empty((Cn - 1) * (2 * K + 1 + 5), dtype=torch.float64, device=dev)
    o = [0, (Cn - 1) * K, 2 * (Cn - 1) * K, (Cn - 1) * (2 * K + 1), (Cn - 1) * (2 * K + 5)]

    def finalize_plain():
        lib.call("dpft_dataset_ap_finalize_f64", rec.data_ptr(), n, start.data_ptr(), st["counters"].data_ptr(), Cn, K, 40,
                 buf[o[0]:].data_ptr(), buf[o[2]:].data_ptr(), buf[o[1]:].data_ptr(), stream())

    def finalize_tp():
        lib.call("dpft_dataset_ap_finalize_tp_f64", rec.data_ptr(), srows.data_ptr(), n, start.data_ptr(), st["counters"].data_ptr(),
                 Cn, tp.tp["k"], 40, tp.tp["i_min"], buf[o[3]:].data_ptr(), buf[o[4]:].data_ptr(), stream())

    emit({"what": "compute() wall clock, ms, with tp_errors beside the compute() without on the same records", "records": n,
          "compute_ms_median without tp_errors": round(statistics.median(walls["plain"]), 2),
          "compute_ms_median with tp_errors": round(statistics.median(walls["tp"]), 2),
          "compute_ms_min without tp_errors": round(min(walls["plain"]), 2), "compute_ms_min with tp_errors": round(min(walls["tp"]), 2),
          "dpft_dataset_ap_finalize_f64 alone": timed(finalize_plain),
          "dpft_dataset_ap_finalize_tp_f64 alone (one workgroup per class)": timed(finalize_tp),
          "gather of the error rows by the sort permutation": timed(lambda: st["tp_errors"][perm].contiguous()),
          "mATE": res["mATE"], "mAZE": res["mAZE"], "mASE": res["mASE"], "mAOE": res["mAOE"], "tp_saturated": res["tp_saturated"]})


def kitti_leg(args, torch, DatasetAP, KINDS, pack_targets, lib, stream, dev, out, labels, B, N, Cn, timed, emit):
    """7. and 8. of the module docstring: an accumulator with the key and one without, fed the same batches in the same process."""
    plain, kitti = DatasetAP(Cn, initial_capacity=1 << 22), DatasetAP(Cn, initial_capacity=1 << 22, kitti=True)
    frame = {"plain": 0, "kitti": 0}

    def update(ap, key):
        def fn():
            ap.update(out, labels, frame[key])
            frame[key] += B
        return fn

    kitti.update(out, labels, 0)
    st = kitti.state()
    K = len(plain.combinations)
    n_det = int(st["counters"][0])
    n_p1 = [int(((st["records"][:, 3] >> (8 + k)) & 1).sum()) for k in range(K)]
    n_p2 = [int(((st["records"][:, 3] >> (16 + k)) & 1).sum()) for k in range(K)]
    kitti.reset()
    t_plain, t_kitti = [], []
    for _ in range(2):                                          # a, b, a, b: the spread of one side beside the difference
        t_plain.append(timed(update(plain, "plain")))
        t_kitti.append(timed(update(kitti, "kitti")))

    # the entries alone, on pre-packed targets
    counts = [int(l["gt_class"].shape[0]) for l in labels]
    gt_box, _, gt_id, counts_t, Mmax = pack_targets(labels, counts, Cn, dev)
    thr = (C.c_double * K)(*[t for _, t in plain.combinations])
    kinds = (C.c_int32 * K)(*[KINDS.index(k) for k, _ in plain.combinations])
    roi = (C.c_float * 6)(*plain.roi)
    scratch = torch.empty(int(lib.dpft_dataset_ap_scratch_bytes(B, N, Mmax)) // 8, dtype=torch.float64, device=dev)
    records = torch.empty((1 << 22, 4), dtype=torch.int32, device=dev)
    counters = torch.zeros(32, dtype=torch.int64, device=dev)
    reserved = [0]
    t4 = [out[k].contiguous() for k in ("class", "center", "size", "angle")]

    def entry(name, *extra):
        def fn():
            if reserved[0] + B * N > records.shape[0]:
                reserved[0] = 0
                counters.zero_()
            lib.call(name, *[t.data_ptr() for t in t4], gt_box.data_ptr(), gt_id.data_ptr(), counts_t.data_ptr(), thr, kinds, K, roi,
                     0.0, scratch.data_ptr(), records.data_ptr(), records.shape[0], reserved[0], counters.data_ptr(), 0, B, N, Mmax,
                     Cn, *extra, stream())
            reserved[0] += B * N
        return fn

    no_groups_no_tp = (None, None, None, None, None, None, 0, None, 0, 0, None, 0, 0)
    e_plain, e_kitti = [], []
    for _ in range(2):
        e_plain.append(timed(entry("dpft_dataset_ap_update_f32")))
        e_kitti.append(timed(entry("dpft_dataset_ap_update_kitti_f32", *no_groups_no_tp)))
    emit({"what": "update with and without kitti, between device events, each side measured twice (a, b, a, b)",
          "device": torch.cuda.get_device_name(0), "B": B, "N": N, "C": Cn, "targets": counts, "K": K,
          "detections_per_update": n_det, "pass1_bits_per_update": n_p1, "pass2_bits_per_update": n_p2, "reps": args.reps,
          "DatasetAP.update without kitti": t_plain, "DatasetAP.update with kitti": t_kitti,
          "dpft_dataset_ap_update_f32 alone": e_plain, "dpft_dataset_ap_update_kitti_f32 alone": e_kitti})

    # compute() on ~ --records records: the same batch under new frame numbers
    plain.reset()
    kitti.reset()
    first = 0
    while plain._bound < args.records * N // max(n_det // B, 1):
        plain.update(out, labels, first)
        kitti.update(out, labels, first)
        first += B
    torch.cuda.synchronize()
    walls = {"plain": [], "kitti": []}
    for _ in range(5):
        for key, ap in (("plain", plain), ("kitti", kitti)):
            t0 = time.perf_counter()
            res = ap.compute()
            walls[key].append((time.perf_counter() - t0) * 1e3)
    assert torch.equal(res["ap"].view(torch.int64), plain.compute()["ap"].view(torch.int64))

    # the finalize entries alone, on the sorted records
    st = kitti.state()
    rec = DatasetAP.sort_records(st["records"])
    n = int(rec.shape[0])
    cls_of = (rec[:, 2] >> 16) & 0xFF
    start = torch.searchsorted(cls_of.contiguous(), torch.arange(Cn + 1, dtype=cls_of.dtype, device=dev)).to(torch.int64)
    cells = (Cn - 1) * K
    buf = torch.empty(cells * (2 + 5 * 41), dtype=torch.float64, device=dev)
    nthr = torch.empty(cells, dtype=torch.int32, device=dev)
    o = [0, cells] + [2 * cells + i * 41 * cells for i in range(5)]

    def finalize_plain():
        lib.call("dpft_dataset_ap_finalize_f64", rec.data_ptr(), n, start.data_ptr(), st["counters"].data_ptr(), Cn, K, 40,
                 buf[o[0]:].data_ptr(), buf[o[2]:].data_ptr(), buf[o[1]:].data_ptr(), stream())

    def finalize_kitti():
        lib.call("dpft_dataset_ap_finalize_kitti_f64", rec.data_ptr(), n, start.data_ptr(), st["counters"].data_ptr(), Cn, K,
                 *[buf[x:].data_ptr() for x in o], nthr.data_ptr(), stream())

    emit({"what": "compute() wall clock, ms, with kitti beside the compute() without on the same records", "records": n,
          "compute_ms_median without kitti": round(statistics.median(walls["plain"]), 2),
          "compute_ms_median with kitti": round(statistics.median(walls["kitti"]), 2),
          "compute_ms_min without kitti": round(min(walls["plain"]), 2), "compute_ms_min with kitti": round(min(walls["kitti"]), 2),
          "dpft_dataset_ap_finalize_f64 alone": timed(finalize_plain),
          "dpft_dataset_ap_finalize_kitti_f64 alone (one workgroup per class and combination, three trips)": timed(finalize_kitti),
          "mAP_3d@0.5": res["mAP_3d@0.5"], "kitti/mAP_3d@0.5": res["kitti/mAP_3d@0.5"], "kitti/mAP11_3d@0.5": res["kitti/mAP11_3d@0.5"],
          "kitti_nthr": res["kitti_nthr"].tolist()})


if __name__ == "__main__":
    main()
