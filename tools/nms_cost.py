"""Cost of the rotated NMS (evaluate.nms), between device events, in one run: the three launches of ``dpft_nms_f32``
(``RotatedNMS.__call__``, which also allocates its outputs and scratch) and the entry alone on pre-allocated buffers, at B = 4,
N = 400, C = 8, beside ``Metric.forward`` and ``DatasetAP.update`` on the same tensors, for three inputs:

  head_like   the tests' seeded sample builder: about 30 targets per frame, every second query a perturbed copy of one
  one_class   every query a candidate of class 1, in dense clusters (nothing is skipped for its class)
  disjoint    every query a candidate, one per cell of a 3 m grid (everything is kept: the scan visits every row)

Prints JSON lines and writes them to ``--out`` (default profiles/nms.txt).
Usage: python tools/nms_cost.py [--reps 200] [--out profiles/nms.txt]

The three launches one by one come from a kernel trace of this script in a run of its own (tracing slows the host: the numbers
above are taken without it):
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/nms_cost.py --reps 50 --out /dev/null
    python tools/nms_cost.py --reps 50 --trace DIR/.../*_kernel_trace.csv --out profiles/nms_kernels.txt      (needs no GPU)
Per input the script runs ``dpft_nms_f32`` 3 * (reps + 10) + 1 times: the trace's NMS kernels are cut into the inputs by that."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


INPUTS = ("head_like", "one_class", "disjoint")


def summarise_trace(args):
    """Median / min / p90 kernel time of the three launches per input, from a rocprofv3 kernel trace of this script."""
    import csv
    per_input = 3 * (args.reps + 10) + 1
    times = {}
    with open(args.trace, newline="") as f:
        for row in sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"])):
            for k in ("nms_sort_kernel", "nms_mask_kernel", "nms_scan_kernel"):
                if k in row["Kernel_Name"]:
                    times.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    lines = []
    for i, name in enumerate(INPUTS):
        d = {"what": "kernel time of the three launches of dpft_nms_f32 (rocprofv3 --kernel-trace, a run of its own), us",
             "input": name, "B": 4, "N": 400, "C": 8, "calls": per_input}
        for k, t in sorted(times.items()):
            assert len(t) == per_input * len(INPUTS), (k, len(t), per_input)
            part = sorted(t[i * per_input:(i + 1) * per_input])
            d[k] = {"median_us": round(statistics.median(part), 1), "min_us": round(part[0], 1),
                    "p90_us": round(part[int(0.9 * len(part))], 1)}
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "nms.txt"))
    p.add_argument("--trace", default=None, help="summarise the rocprofv3 kernel trace (csv) of a run with the same --reps")
    args = p.parse_args()
    if args.trace is not None:
        return summarise_trace(args)
    import numpy as np
    import torch
    from tests import dataset_ap_ref as G                       # the tests' seeded sample builders
    from tests import nms_ref as R
    from dpft_amd.evaluation.dataset_ap import DatasetAP
    from dpft_amd.evaluation.metric import Metric
    from dpft_amd.evaluation.nms import RotatedNMS
    from dpft_amd.hip.lib import lib, stream

    assert torch.cuda.is_available(), "nms_cost.py measures on the GPU; there is nothing to measure without one"
    dev = torch.device("cuda", 0)
    B, N, Cn = 4, 400, 8
    rng = np.random.default_rng(0)
    head = [G.random_sample(rng, N, int(m), Cn) for m in rng.integers(26, 35, B)]
    labels = [{k: torch.from_numpy(s[k]).to(dev) for k in ("gt_center", "gt_size", "gt_angle", "gt_class")} for s in head]
    one = [R.layout_frame(rng, N, N, 2, "dense") for _ in range(B)]
    for f in one:                                                # the same scores in 8 columns: class 1 everywhere
        f["cls"] = np.concatenate([f["cls"], np.full((N, Cn - 2), -9.0, dtype=np.float32)], 1)
    inputs = dict(zip(INPUTS, (head, one, [R.layout_frame(rng, N, N, Cn, "disjoint") for _ in range(B)])))
    nms = RotatedNMS()                                           # the defaults: bev, IoU 0.3, class-aware
    ap = DatasetAP(Cn, initial_capacity=1 << 22)                 # (no growth inside the timed region)
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

    for name, frames in inputs.items():
        out = {k: torch.from_numpy(np.stack([f[src] for f in frames])).to(dev)
               for k, src in (("class", "cls"), ("center", "center"), ("size", "size"), ("angle", "angle"))}
        status, order, counts, cls_out = nms(out)
        scratch = torch.empty((int(lib.dpft_nms_scratch_bytes(B, N)) + 7) // 8, dtype=torch.int64, device=dev)
        thr = (C.c_double * 1)(nms.iou)
        t4 = [out[k].contiguous() for k in ("class", "center", "size", "angle")]

        def alone():
            lib.call("dpft_nms_f32", *[t.data_ptr() for t in t4], thr, 0, 0, -math.inf, 0x7FFFFFFF, scratch.data_ptr(),
                     status.data_ptr(), order.data_ptr(), counts.data_ptr(), cls_out.data_ptr(), B, N, Cn, stream())

        frame = [0]

        def update():
            ap.update(out, labels, frame[0])
            frame[0] += B

        ap.reset()
        st = status.cpu().numpy()
        emit({"what": "rotated NMS beside Metric.forward and DatasetAP.update, between device events", "input": name,
              "device": torch.cuda.get_device_name(0), "B": B, "N": N, "C": Cn, "reps": args.reps,
              "candidates": [int((s != -2).sum()) for s in st], "kept": counts.cpu().tolist(),
              "RotatedNMS.__call__": timed(lambda: nms(out)), "dpft_nms_f32 alone (3 launches)": timed(alone),
              "RotatedNMS.suppress + Metric.forward": timed(lambda: metric(nms.suppress(out), labels)),
              "Metric.forward": timed(lambda: metric(out, labels)), "DatasetAP.update": timed(update)})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
