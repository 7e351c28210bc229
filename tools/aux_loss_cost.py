"""Cost of deep supervision (train.aux_loss, DESIGN.md 3 "Deep supervision").

1. The loss section alone, between device events with warm-up, at the kradar loss shape (the built-in config's batch 4 and
   400 queries, the bench's synthetic labels): today's entries on one output (dpft_match_cost_f32 + dpft_assign_loss_dev_f32
   with its gradient launch) against the layered entries (dpft_match_cost_layers_f32 + dpft_assign_loss_layers_dev_f32) at
   L = 1 and L = 4, alternating in one process -- every repetition times the three forms one after the other.
2. Same-box pairs (``--pairs n``: n alternating pairs) of ``bench.py --gpus 1 --steps K --warmup W`` lines, key absent against
   ``"aux_loss": true`` (through ``--config`` with the built-in kradar config written out plus the key), each in a child
   process of its own.  ``--no-bench`` skips this part.  Without it, part 1 runs in a child process as well (this file with
   ``--no-bench``), so that the process which waits for bench.py never opens the device.

Prints one JSON line per part.  Usage: python tools/aux_loss_cost.py [--reps 200] [--steps 100] [--warmup 20] [--pairs 1]"""
import argparse
import ctypes as C
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


def loss_section_alone(args):
    """Part 1, in this process."""
    import torch
    from dpft_amd.hip.lib import lib, stream
    from dpft_amd.synthetic import make_labels
    from dpft_amd.training.loss import _layer_table, pack_targets

    assert torch.cuda.is_available(), "aux_loss_cost.py measures on the GPU; there is nothing to measure without one"
    cfg = load_config("kradar")
    B, N = cfg["train"]["batch_size"], cfg["model"]["fuser"]["n_queries"]
    ncls = cfg["model"]["head"]["num_classes"]
    lw = cfg["train"]["loss_weights"]
    dev = torch.device("cuda", 0)
    labels = make_labels(B, seed=cfg["computing"]["seed"], device=dev)      # (bench.py's labels)
    counts = [int(t["gt_class"].shape[0]) for t in labels]
    gt_box, gt_onehot, gt_id, counts_t, Mmax = pack_targets(labels, counts, ncls, dev)
    g = torch.Generator().manual_seed(0)
    LMAX = 4

    def output():
        o = {"class": torch.randn(B, N, ncls, generator=g),
             "center": torch.randn(B, N, 3, generator=g) * torch.tensor([20.0, 4.0, 1.0]) + torch.tensor([35.0, 0, 0]),
             "size": torch.relu(torch.randn(B, N, 3, generator=g) + 2.0), "angle": torch.tanh(torch.randn(B, N, 2, generator=g))}
        return tuple(o[k].to(dev) for k in ("class", "center", "size", "angle"))
    tens = [output() for _ in range(LMAX)]
    grads = [tuple(torch.empty_like(t) for t in tl) for tl in tens]
    terms = ("total_class", "object_class", "center", "size", "angle")
    w5 = (C.c_float * 5)(*(float(lw.get(k, 0.0)) for k in terms))
    cw = (C.c_float * 5)(lw["total_class"], lw["center"], lw["size"], lw["angle"], 1.0)
    sel = torch.tensor([1.0 if k in lw else 0.0 for k in terms], device=dev)
    cost = torch.empty((LMAX, B, N, Mmax), device=dev)
    tiled = torch.empty(LMAX * B, dtype=torch.int32, device=dev)
    packed = torch.empty(LMAX * B * Mmax * 2 + LMAX * B, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = torch.zeros(int(lib.dpft_set_loss_layers_scratch_floats(LMAX, B, N)) + 1024, device=dev)
    losses, layer_totals, total = torch.empty((LMAX, 5), device=dev), torch.empty(LMAX, device=dev), torch.empty((), device=dev)
    tables = {L: _layer_table(tens[:L], [1.0] * L, grads[:L]) for L in (1, LMAX)}

    def single():
        cls, center, size, angle = tens[0]
        dcls, dcenter, dsize, dangle = grads[0]
        lib.call("dpft_match_cost_f32", cls.data_ptr(), center.data_ptr(), size.data_ptr(), angle.data_ptr(), gt_box.data_ptr(),
                 gt_id.data_ptr(), counts_t.data_ptr(), C.byref(cw), cost.data_ptr(), B, N, Mmax, ncls, stream())
        lib.call("dpft_assign_loss_dev_f32", cost.data_ptr(), counts_t.data_ptr(), packed.data_ptr(), status.data_ptr(),
                 cls.data_ptr(), center.data_ptr(), size.data_ptr(), angle.data_ptr(), gt_box.data_ptr(), gt_onehot.data_ptr(),
                 C.cast(w5, C.c_void_p), 0.75, sel.data_ptr(), scratch.data_ptr(), losses.data_ptr(), total.data_ptr(),
                 dcls.data_ptr(), dcenter.data_ptr(), dsize.data_ptr(), dangle.data_ptr(), B, N, Mmax, ncls, stream())

    def layered(L):
        def run():
            lib.call("dpft_match_cost_layers_f32", tables[L], L, gt_box.data_ptr(), gt_id.data_ptr(), counts_t.data_ptr(),
                     C.byref(cw), cost.data_ptr(), tiled.data_ptr(), B, N, Mmax, ncls, stream())
            lib.call("dpft_assign_loss_layers_dev_f32", cost.data_ptr(), tiled.data_ptr(), packed.data_ptr(), status.data_ptr(),
                     tables[L], L, gt_box.data_ptr(), gt_onehot.data_ptr(), C.cast(w5, C.c_void_p), 0.75, sel.data_ptr(),
                     scratch.data_ptr(), losses.data_ptr(), layer_totals.data_ptr(), total.data_ptr(), B, N, Mmax, ncls, stream())
        return run
    forms = {"single": single, "layers_L1": layered(1), f"layers_L{LMAX}": layered(LMAX)}
    for _ in range(20):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    events = []
    for _ in range(args.reps):
        for k, fn in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            events.append((k, a, b))
    torch.cuda.synchronize()
    assert int(status) == 0
    for k, a, b in events:
        times[k].append(a.elapsed_time(b) * 1e3)

    def stats(t):
        t = sorted(t)
        return {"median_us": round(statistics.median(t), 1), "min_us": round(t[0], 1), "p90_us": round(t[int(0.9 * len(t))], 1)}
    res = {k: stats(t) for k, t in times.items()}
    print(json.dumps({"what": "loss section alone (cost + assignment + criterion + gradient; four launches, two C calls), between "
                              "device events, the three forms alternating", "device": torch.cuda.get_device_name(0), "B": B, "N": N,
                      "Mmax": Mmax, "targets": counts, "reps": args.reps, **res,
                      f"L{LMAX}_over_{LMAX}x_single": round(res[f"layers_L{LMAX}"]["median_us"] / (LMAX * res["single"]["median_us"]), 3),
                      "L1_over_single": round(res["layers_L1"]["median_us"] / res["single"]["median_us"], 3)}), flush=True)


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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=1, help="bench.py pairs, alternating key absent / key present")
    ap.add_argument("--no-bench", action="store_true")
    args = ap.parse_args()
    if args.no_bench:
        loss_section_alone(args)
        return
    print(json.dumps(child("loss section alone", [sys.executable, os.path.abspath(__file__), "--no-bench", "--reps",
                                                  str(args.reps)])), flush=True)
    cfg = load_config("kradar")
    cfg["train"]["aux_loss"] = True
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "kradar_aux.json")
        with open(path, "w") as f:
            json.dump(cfg, f)
        for label, extra in (("key absent", []), ("key present", ["--config", path])) * args.pairs:
            line = child("bench, " + label, [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                                             str(args.steps), "--warmup", str(args.warmup), "--no-secondary",
                                             "--no-cpu-baseline"] + extra)
            print(json.dumps({"bench": label, "aux_loss": bool(extra), **{k: line[k] for k in KEEP if k in line}}), flush=True)


if __name__ == "__main__":
    main()
