"""Cost of the test-time-augmentation fusion (evaluate.tta), between device events, in one run: ``fuse`` as a whole
(allocations, gather, the three launches of ``dpft_nms_f32`` on the union, vote) and its gather and vote launches alone on
pre-allocated buffers, beside ``RotatedNMS`` on one view's N queries and ``Metric.forward`` on the fused (B, T N) tensors, at
batch 4, 8 classes, on a seeded head-like output (the tests' view builder: every view sees the same objects with its own noise,
two thirds of the queries are candidates):

  T = 2 at N = 400 queries (the model's own number: 800 candidates)
  T = 4 at N = 256 queries (T N <= 1024: four views of 400 queries are refused)

and one line for ``evaluate_one_epoch`` per batch with and without the key: the model of ``smoke()`` (ResNet-50 bodies, small
frames, 400 queries, batch 4, random weights), the per-step metrics, wall clock around a synchronised epoch of 8 batches.

Prints JSON lines and writes them to ``--out`` (default profiles/tta.txt).
Usage: python tools/tta_cost.py [--reps 200] [--out profiles/tta.txt]"""
import argparse
import copy
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "tta.txt"))
    args = p.parse_args()
    import numpy as np
    import torch
    from tests import dataset_ap_ref as G                       # the tests' seeded builders
    from tests import tta_ref as R
    from dpft_amd.evaluation.metric import Metric
    from dpft_amd.evaluation.nms import RotatedNMS
    from dpft_amd.evaluation.tta import TestTimeAugmentation
    from dpft_amd.hip.lib import TtaViews, lib, stream

    assert torch.cuda.is_available(), "tta_cost.py measures on the GPU; there is nothing to measure without one"
    dev = torch.device("cuda", 0)
    B, Cn = 4, 8
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

    metric = Metric(metrics={"mAP": "mAP3D", "mGIoU": "mGIoU3D"})
    for T, N in ((2, 400), (4, 256)):
        rng = np.random.default_rng(T)
        flips = tuple([False] + [t % 2 == 1 for t in range(1, T)])
        per_frame = [R._view_frames(rng, N, Cn, T, flips, "mixed") for _ in range(B)]
        outs = [{k: torch.from_numpy(np.stack([per_frame[b][t][src] for b in range(B)])).to(dev)
                 for k, src in (("class", "cls"), ("center", "center"), ("size", "size"), ("angle", "angle"))} for t in range(T)]
        labels = [{k: torch.from_numpy(s[k]).to(dev) for k in ("gt_center", "gt_size", "gt_angle", "gt_class")}
                  for s in (G.random_sample(rng, N, int(m), Cn) for m in rng.integers(26, 35, B))]
        tta = TestTimeAugmentation(views=[{"flip": True} if f else {"zoom": 1.1} for f in flips[1:]])
        nms = RotatedNMS()
        fused = tta.fuse(outs)
        status, order, counts, members = tta.clusters(outs)
        M = T * N
        f32 = dict(dtype=torch.float32, device=dev)
        union = [torch.empty((B, M, w), **f32) for w in (Cn, 3, 3, 2)]
        res = [torch.empty((B, M, w), **f32) for w in (Cn, 3, 3, 2)]
        scratch = torch.empty((int(lib.dpft_tta_scratch_bytes(B, N, T)) + 7) // 8, dtype=torch.int64, device=dev)
        mem = torch.empty((B, M), dtype=torch.int32, device=dev)
        table = TtaViews()
        for t, o in enumerate(outs):
            table.cls[t], table.center[t], table.size[t], table.angle[t] = (o[k].data_ptr() for k in ("class", "center", "size", "angle"))
            table.flip[t] = int(flips[t])
        thr = (C.c_double * 1)(tta.iou)

        def gather():
            lib.call("dpft_tta_gather_f32", C.byref(table), T, *(u.data_ptr() for u in union), B, N, Cn, stream())

        def cluster():
            lib.call("dpft_nms_f32", *(u.data_ptr() for u in union), thr, 0, 0, 0.0, 0x7FFFFFFF, scratch.data_ptr(), status.data_ptr(),
                     order.data_ptr(), counts.data_ptr(), res[0].data_ptr(), B, M, Cn, stream())

        def vote():
            lib.call("dpft_tta_vote_f32", union[1].data_ptr(), union[2].data_ptr(), union[3].data_ptr(), status.data_ptr(),
                     scratch.data_ptr(), 0, T, res[0].data_ptr(), res[1].data_ptr(), res[2].data_ptr(), res[3].data_ptr(),
                     mem.data_ptr(), B, N, Cn, stream())

        gather()
        cluster()
        vote()
        torch.cuda.synchronize()
        assert all(torch.equal(a.view(torch.int32), fused[k].view(torch.int32)) for a, k in zip(res, ("class", "center", "size", "angle")))
        st = status.cpu().numpy()
        emit({"what": "TTA fusion beside RotatedNMS and Metric.forward, between device events", "device": torch.cuda.get_device_name(0),
              "B": B, "N": N, "T": T, "C": Cn, "reps": args.reps, "candidates": [int((s != -2).sum()) for s in st],
              "heads": counts.cpu().tolist(), "largest_cluster": int(members.max()),
              "TestTimeAugmentation.fuse (5 launches + allocations)": timed(lambda: tta.fuse(outs)),
              "dpft_tta_gather_f32 alone": timed(gather), "dpft_nms_f32 on the union alone (3 launches)": timed(cluster),
              "dpft_tta_vote_f32 alone": timed(vote), f"RotatedNMS.__call__ on one view (N = {N})": timed(lambda: nms(outs[0])),
              f"Metric.forward on the fused output (B, {M})": timed(lambda: metric(fused, labels)),
              f"Metric.forward on one view (B, {N})": timed(lambda: metric(outs[0], labels))})

    # ---- evaluate_one_epoch per batch, with and without the key ----
    from dpft_amd.configs import load_config
    from dpft_amd.evaluation import DataParallelEvaluator
    from dpft_amd.models import build as build_model
    from dpft_amd.synthetic import make_batch, make_labels
    cfg = copy.deepcopy(load_config("kradar"))
    cfg["model"]["backbones"]["camera_mono"]["name"] = "ResNet50"
    torch.manual_seed(0)
    model = build_model("dprt", cfg).to(dev).eval()
    shapes = {"camera_mono": (64, 96, 3), "radar_bev": (64, 43, 6), "radar_front": (37, 43, 6)}
    batch = {k: v.to(dev) for k, v in make_batch(cfg["model"]["inputs"], B, seed=1, shapes=shapes).items()}
    labels = make_labels(B, seed=1, device=dev)
    loader = [(batch, labels)] * 8
    per_batch = {}
    for name, tta in (("without evaluate.tta", None), ("evaluate.tta: true (T = 2)", TestTimeAugmentation())):
        ev = DataParallelEvaluator(metric=metric, device=dev, tta=tta)
        ev.evaluate_one_epoch(0, model, loader[:2])
        t = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev.evaluate_one_epoch(0, model, loader)
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) / len(loader) * 1e3)
        per_batch[name] = {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3)}
    emit(dict({"what": "evaluate_one_epoch per batch (forward(s) + fusion + Metric.forward), wall clock over 8 batches, 5 epochs",
               "model": "smoke() model: ResNet-50 bodies, frames 64x96 / 64x43 / 37x43, 400 queries, random weights", "B": B}, **per_batch))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
