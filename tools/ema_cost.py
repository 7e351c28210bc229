"""Cost of train.ema inside the fused AdamW launch on the full-size kradar model ("EMA of the weights").

One trainer, built as the tests build it (graphs enabled), stepped a few times so that tables, moments and gradients exist; then
the optimizer launch alone (FusedAdamW.launch_tables, one launch per group's table: dpft_adamw_f32 with the EMA off, dpft_adamw_ema_f32 with
it on) between device events, in alternating blocks, and the dpft_swap_f32 launch of swap_ema() the same way.
Every timed repetition is a real update (FusedAdamW.launch_tables) with the gradients the last train_step left: the weights of
this throw-away trainer drift, which does not change what the launch streams.  Each "on" block allocates and seeds the EMA
buffer anew (set_ema), outside the timed window.
Prints one JSON line.  Usage: python tools/ema_cost.py [--reps 50] [--blocks 4] [--batch 4] [--decay 0.999]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpft_amd.configs import load_config                      # noqa: E402
from dpft_amd.models import build                             # noqa: E402
from dpft_amd.synthetic import make_batch, make_labels        # noqa: E402
from dpft_amd.training.trainer import DataParallelTrainer     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--blocks", type=int, default=4)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--decay", type=float, default=0.999)
args = ap.parse_args()

assert torch.cuda.is_available(), "ema_cost.py measures on the GPU; there is nothing to measure without one"
cfg = load_config("kradar")
torch.manual_seed(0)
dev = torch.device("cuda", 0)
tr = DataParallelTrainer(build("dprt", cfg), cfg, dev)
data = make_batch(cfg["model"]["inputs"], args.batch, device=dev)
labels = make_labels(args.batch, device=dev)
tr.enable_graphs(data)
opt = tr.optimizer
for _ in range(3):
    tr.train_step(data, labels)
torch.cuda.synchronize()
seen = tr.reducer.seen_ids()                                  # the parameters the last step updated
trainable = [p for g in opt.param_groups for p in g["params"] if p.requires_grad]
n_elem = sum(p.numel() for p in trainable if p.grad is not None and id(p) in seen)
n_all = sum(p.numel() for p in trainable)


def timed(fn):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
    for _ in range(5):
        fn()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3


us = {False: [], True: []}
for _ in range(args.blocks):
    for on in (False, True):
        opt.set_ema(args.decay if on else None)
        us[on].append(timed(opt.launch_tables))
opt.set_ema(args.decay)
swap = timed(opt.swap_ema)
off, on = statistics.median(us[False]), statistics.median(us[True])
print(json.dumps({
    "what": "the fused AdamW launch with train.ema off / on, kradar", "device": torch.cuda.get_device_name(0),
    "batch": args.batch, "reps_per_block": args.reps, "active_elements": n_elem, "trainable_elements": n_all,
    "adamw_us_off": [round(x, 1) for x in us[False]], "adamw_us_on": [round(x, 1) for x in us[True]],
    "median_us_off": round(off, 1), "median_us_on": round(on, 1), "extra_us": round(on - off, 1),
    "bytes_off": 28 * n_elem, "bytes_on": 36 * n_elem,             # 4 reads + 3 writes -> 5 reads + 4 writes of 4 bytes
    "GBps_off": round(28 * n_elem / (off * 1e-6) / 1e9, 1), "GBps_on": round(36 * n_elem / (on * 1e-6) / 1e9, 1),
    "extra_us_at_off_rate": round(8 * n_elem / (28 * n_elem / off), 1),
    "swap_us": round(swap, 1), "swap_GBps": round(16 * n_all / (swap * 1e-6) / 1e9, 1)}))
