"""Cost of the criterion's optional GIoU3D term (train.loss_weights["giou"]).

1. The two entries alone, between device events, at the kradar loss shape: the built-in config's batch 4 and query count
   (400), about 30 targets per sample, every target matched.  dpft_giou_loss_fwd_f32, and dpft_giou_loss_bwd_f32 in the
   accumulate form (what a training step launches).
2. A same-box pair (``--pairs n``: n alternating pairs) of ``bench.py --gpus 1 --steps K --warmup W`` lines, key absent
   against key present (the second one through ``--config`` with the built-in kradar config written out plus the key),
   each in a child process of its own.  ``--no-bench`` skips this part.  Without it, part 1 runs in a child process as well
   (this file with ``--no-bench``), so that the process which waits for bench.py never opens the device.

Prints one JSON line per part.  Usage: python tools/giou_loss_cost.py [--reps 200] [--steps 100] [--warmup 20] [--weight 2.0] [--pairs 1]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dpft_amd.configs import load_config                      # noqa: E402

KEEP = ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "step_ms_min", "step_ms_median", "step_ms_max", "dtype")


def kernels_alone(args):
    """Part 1, in this process."""
    import numpy as np
    import torch
    from dpft_amd.hip.lib import lib, stream

    assert torch.cuda.is_available(), "giou_loss_cost.py measures on the GPU; there is nothing to measure without one"
    cfg = load_config("kradar")
    B, N = cfg["train"]["batch_size"], cfg["model"]["fuser"]["n_queries"]
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    counts = rng.integers(args.targets - 4, args.targets + 5, B)
    Mmax = int(counts.max())

    def f32(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)

    # boxes the size of the labels of dpft_amd.synthetic.make_labels; every prediction a perturbed copy of "its" target, so
    # that most matched pairs overlap (the clip runs through all its branches)
    gt = np.zeros((B, Mmax, 8), dtype=np.float32)
    gt[..., 0:3] = rng.uniform((5, -6, -1.5), (70, 6, 2), (B, Mmax, 3))
    gt[..., 3:6] = rng.uniform((3.5, 1.6, 1.4), (5.0, 2.2, 2.0), (B, Mmax, 3))
    yaw = rng.uniform(-np.pi, np.pi, (B, Mmax))
    gt[..., 6], gt[..., 7] = np.sin(yaw), np.cos(yaw)
    center = rng.uniform((5, -6, -1.5), (70, 6, 2), (B, N, 3))
    size = rng.uniform((3.5, 1.6, 1.4), (5.0, 2.2, 2.0), (B, N, 3))
    angle = rng.standard_normal((B, N, 2))
    match = np.full((B, Mmax, 2), -1, dtype=np.int32)
    for b in range(B):
        rows = rng.permutation(N)[:counts[b]]
        for k, i in enumerate(rows):
            match[b, k] = (i, k)
            center[b, i] = gt[b, k, 0:3] + rng.normal(0, 0.5, 3)
            size[b, i] = gt[b, k, 3:6] * rng.uniform(0.8, 1.2, 3)
            angle[b, i] = gt[b, k, 6:8] + rng.normal(0, 0.2, 2)
    center, size, angle, gt_box = f32(center), f32(size), f32(angle), f32(gt)
    match_t = torch.from_numpy(match).to(dev)
    counts_t = torch.from_numpy(counts.astype(np.int32)).to(dev)
    total_in = torch.ones((), device=dev)
    term, total = torch.empty((), device=dev), torch.empty((), device=dev)
    G = torch.empty((B, Mmax), device=dev)
    grads = [torch.zeros_like(t) for t in (center, size, angle)]
    head = (center.data_ptr(), size.data_ptr(), angle.data_ptr(), gt_box.data_ptr(), match_t.data_ptr(), counts_t.data_ptr(),
            args.weight)

    def fwd(per_pair=None):
        lib.call("dpft_giou_loss_fwd_f32", *head, total_in.data_ptr(), term.data_ptr(), total.data_ptr(), per_pair, B, N, Mmax,
                 stream())

    def bwd():
        lib.call("dpft_giou_loss_bwd_f32", *head, None, grads[0].data_ptr(), grads[1].data_ptr(), grads[2].data_ptr(), 1, B, N,
                 Mmax, stream())

    def timed(fn):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for _ in range(10):
            fn()
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
        return {"median_us": round(statistics.median(t), 1), "min_us": round(t[0], 1), "p90_us": round(t[int(0.9 * len(t))], 1)}

    fwd(G.data_ptr())
    overlapping = int(((G > -0.5) & (torch.arange(Mmax, device=dev)[None] < counts_t[:, None])).sum())
    print(json.dumps({"what": "dpft_giou_loss_fwd_f32 / dpft_giou_loss_bwd_f32 (accumulate) alone, between device events",
                      "device": torch.cuda.get_device_name(0), "B": B, "N": N, "Mmax": Mmax, "pairs": int(counts.sum()),
                      "pairs_with_G_above_-0.5": overlapping, "term": round(float(term), 6), "reps": args.reps,
                      "fwd": timed(fwd), "bwd": timed(bwd)}), flush=True)


def child(label, cmd):
    """One child process; its last JSON line, or exit with what it left on stderr."""
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    lines = [l for l in res.stdout.strip().splitlines() if l.startswith("{")]
    if res.returncode != 0 or not lines:
        print(json.dumps({"part": label, "failed": res.returncode, "stderr": res.stderr[-2000:]}), flush=True)
        sys.exit(1)
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--targets", type=int, default=30)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--weight", type=float, default=2.0)
    ap.add_argument("--pairs", type=int, default=1, help="bench.py pairs, alternating key absent / key present")
    ap.add_argument("--no-bench", action="store_true")
    args = ap.parse_args()
    if args.no_bench:
        kernels_alone(args)
        return
    print(json.dumps(child("kernels alone", [sys.executable, os.path.abspath(__file__), "--no-bench", "--reps", str(args.reps),
                                             "--targets", str(args.targets), "--weight", str(args.weight)])), flush=True)
    cfg = load_config("kradar")
    cfg["train"]["loss_weights"]["giou"] = args.weight
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "kradar_giou.json")
        with open(path, "w") as f:
            json.dump(cfg, f)
        for label, extra in (("key absent", []), ("key present", ["--config", path])) * args.pairs:
            line = child("bench, " + label, [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                                             str(args.steps), "--warmup", str(args.warmup), "--no-secondary",
                                             "--no-cpu-baseline"] + extra)
            print(json.dumps({"bench": label, "weight": None if not extra else args.weight,
                              **{k: line[k] for k in KEEP if k in line}}), flush=True)


if __name__ == "__main__":
    main()
