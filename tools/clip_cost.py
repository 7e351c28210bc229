"""Cost of train.clip_grad_norm on the kradar batch-4 training step ("Gradient clipping").

One trainer, built as the tests build it (graphs enabled), stepped in alternating blocks with clipping off and on (the
optimizer's set_clip toggled between blocks: the launches of a block are those of a trainer built with / without the key), each
block timed by a host clock around a device synchronise; then the two norm launches alone between device events.
Prints one JSON line.  Usage: python tools/clip_cost.py [--blocks 6] [--steps 20] [--batch 4]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpft_amd.configs import load_config                      # noqa: E402
from dpft_amd.hip.lib import lib, ptr, stream                 # noqa: E402
from dpft_amd.models import build                             # noqa: E402
from dpft_amd.synthetic import make_batch, make_labels        # noqa: E402
from dpft_amd.training.trainer import DataParallelTrainer     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=6)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--max-norm", type=float, default=0.1)
args = ap.parse_args()

assert torch.cuda.is_available(), "clip_cost.py measures on the GPU; there is nothing to measure without one"
cfg = load_config("kradar")
cfg["train"]["clip_grad_norm"] = args.max_norm
torch.manual_seed(0)
dev = torch.device("cuda", 0)
tr = DataParallelTrainer(build("dprt", cfg), cfg, dev)
data = make_batch(cfg["model"]["inputs"], args.batch, device=dev)
labels = make_labels(args.batch, device=dev)
tr.enable_graphs(data)
opt = tr.optimizer


def block(clip: bool) -> float:
    opt.set_clip(args.max_norm if clip else None)
    tr.clip = (args.max_norm, "propagate") if clip else None
    tr.train_step(data, labels)                               # (the first step after a toggle is not timed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        tr.train_step(data, labels)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.steps * 1e3


for clip in (False, True):                                    # warm-up of both forms
    block(clip)
times = {False: [], True: []}
for _ in range(args.blocks):
    for clip in (False, True):
        times[clip].append(block(clip))

# the two norm launches alone (the tables and gradients of the last clipped step)
opt.set_clip(args.max_norm)
tr.train_step(data, labels)
torch.cuda.synchronize()
n_rows = sum(tb["n_chunks"] for tb in opt._tables)
n_elem = sum(p.numel() for tb in opt._tables for p, a in zip(tb["params"], tb["active_host"]) if a)


def timed(fn, reps=50):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for _ in range(5):
        fn()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return {"median_us": 1e3 * statistics.median(ms), "min_us": 1e3 * ms[0], "max_us": 1e3 * ms[-1]}


def stage1():
    for tb in opt._tables:
        lib.call("dpft_grad_sqnorm_f32", ptr(tb["chunks"]), tb["n_chunks"], ptr(tb["active"]),
                 C.c_void_p(opt._partials.data_ptr() + 8 * tb["part_off"]), stream())


def stage2():
    lib.call("dpft_grad_clip_coef_f32", ptr(opt._partials), opt._partials.numel(), args.max_norm, 0, ptr(opt._clip_record),
             stream())


s1, s2, both = timed(stage1), timed(stage2), timed(opt._launch_norm)
print(json.dumps({
    "what": "train.clip_grad_norm on the kradar training step", "batch": args.batch, "steps_per_block": args.steps,
    "step_ms_without": [round(x, 3) for x in times[False]], "step_ms_with": [round(x, 3) for x in times[True]],
    "median_without_ms": round(statistics.median(times[False]), 3), "median_with_ms": round(statistics.median(times[True]), 3),
    "rows": n_rows, "active_elements": n_elem, "grad_bytes": 4 * n_elem,
    "sqnorm": s1, "clip_coef": s2, "both_launches": both,
    "sqnorm_GBps": round(4 * n_elem / (s1["median_us"] * 1e-6) / 1e9, 1),
    "grad_norm": float(tr.last_grad_norm)}))
