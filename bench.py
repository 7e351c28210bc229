#!/usr/bin/env python
"""Headline benchmark: training samples/s of the full camera+radar DPFT hot path (config kradar,
batch 4 per GPU, fp32, synthetic K-Radar-shaped tensors resident in HBM), plus fwd ms/frame.

    python bench.py --gpus 1 --steps 100 --warmup 20
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A step = zero-grad -> forward -> Hungarian set loss -> backward -> (bucketed all-reduce) -> AdamW,
the reference's CentralizedTrainer.train_one_epoch order (src/dprt/training/trainer.py:99-160).
Rank 0 prints ONE JSON line (see DESIGN.md "Measurement").
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
# kernel arguments in device memory: the ROCm 7.2 default on gfx950, pinned here because the step is ~960 dependent
# launches on one stream (HIP_FORCE_DEV_KERNARG=0 measures 41.5 instead of 38.9 ms per step)
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

import torch
import torch.distributed as dist

PEAK_F32_MFMA_TFLOPS = 157.3       # /opt/skills/guides/MI355X_MICROARCH.md, chip table
PEAK_BF16_MFMA_TFLOPS = 2500.0     # dense bf16 (same table); only used by --dtype bf16


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)      # SURVEY 8d / BASELINE.md: 20 warm-up + >= 100 timed steps
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4, help="per-GPU batch (BASELINE: 4)")
    ap.add_argument("--config", default="kradar")
    ap.add_argument("--latency-reps", type=int, default=300,
                    help="event-timed eval forwards for fwd ms/frame (reference protocol: 10 warm-up + 300)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16", "f32x3"],
                    help="f32 = the reference's arithmetic (BASELINE metric, default); bf16 = mixed precision of "
                         "BASELINE.json configs[4]: bf16 operands / fp32 accumulation in the conv GEMMs")
    ap.add_argument("--no-split", action="store_true",
                    help="f32 only: v_mfma_f32_32x32x2_f32 everywhere (default: the big multi-tap conv GEMMs run as 3 x bf16 split "
                         "products on the bf16 matrix cores -- fp32 in, fp32 out, dpft_conv_set_split)")
    ap.add_argument("--no-graphs", action="store_true", help="do not replay the decoder from hipGraphs")
    ap.add_argument("--bucket-mb", type=float, default=None, help="gradient bucket size (default 25 MiB)")
    ap.add_argument("--comm-dtype", default=None, choices=[None, "fp32", "bf16"], help="wire format of the gradient all-reduce")
    ap.add_argument("--force-collectives", action="store_true",
                    help="N=1 only: run the N>1 exchange path (RCCL communicator of one rank, every bucket through "
                         "dist.all_reduce on RCCL's stream, all-ranks step decision) on the single GPU")
    ap.add_argument("--cpu-threads", type=int, default=0, help="0 = all host cores (BASELINE.md section 3)")
    ap.add_argument("--cpu-timeout", type=int, default=120, help="wall-clock budget of the CPU baseline leg in s")
    ap.add_argument("--cpu-baseline-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-secondary", action="store_true",
                    help="skip the secondary legs (BASELINE.json configs[1] radar-BEV batch 4 and configs[4] bf16 batch 8)")
    ap.add_argument("--leg", action="store_true", help=argparse.SUPPRESS)      # child mode of secondary_legs(): compact line
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure what the headline does not need: the conv roofline (serialized "
                         "step), the loss window, eval-forward latency, the decoder rooflines, the CPU baseline and the "
                         "secondary legs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy (see dump_outputs)")
    return ap.parse_args()


def cpu_model_name() -> str:
    """'model name' of /proc/cpuinfo (+ socket count); platform.processor() only says 'x86_64' on Linux."""
    import platform
    try:
        names, sockets = [], set()
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.startswith("model name"):
                    names.append(ln.split(":", 1)[1].strip())
                elif ln.startswith("physical id"):
                    sockets.add(ln.split(":", 1)[1].strip())
        if names:
            return f"{names[0]} ({len(names)} logical CPUs, {max(len(sockets), 1)} socket(s))"
    except OSError:
        pass
    return platform.processor() or platform.machine()


def cpu_baseline(threads: int = 0, budget_s: float = 200.0):
    """The oracle (CPU restatement of the reference path, torch fp32; pinned to the imported reference by
    tests/test_oracle_golden.py) timed on the host cores with the protocol of BASELINE.md section 3: configs 1-3,
    forward 2 warm-up + 5 timed, train step (forward + Hungarian set loss + backward + AdamW) 1 warm-up + 3 timed,
    ``torch.set_num_threads(all host cores)``.  ``budget_s`` bounds the sample: a leg that would not fit is cut to
    fewer timed repetitions (reported)."""
    from dpft_amd.configs import load_config
    from dpft_amd.models import build
    from dpft_amd.synthetic import make_batch, make_labels
    from oracle import dprt_oracle as O
    t_begin = time.perf_counter()
    host = os.cpu_count() or 1
    if threads > 0:
        cores = threads
    else:
        # all host cores is the protocol's intent, but torch's CPU convolutions stop scaling (and then thrash) long before
        # 256 threads: time one layer-3 sized 3x3 convolution at a few thread counts and keep the fastest
        x, w = torch.randn(4, 256, 32, 57), torch.randn(256, 256, 3, 3)
        best = None
        for n in sorted({min(host, c) for c in (16, 32, 64, 128, host)}):
            torch.set_num_threads(n)
            torch.nn.functional.conv2d(x, w, padding=1)
            t0 = time.perf_counter()
            for _ in range(3):
                torch.nn.functional.conv2d(x, w, padding=1)
            dt = time.perf_counter() - t0
            if best is None or dt < best[0]:
                best = (dt, n)
        cores = best[1]
    torch.set_num_threads(cores)
    legs = {}

    def state(cfg):
        torch.manual_seed(0)
        model = build("dprt", cfg)
        sd = {k: (v.detach().clone().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.detach())
              for k, v in model.state_dict().items()}
        return sd

    def timed(fn, warm, reps):
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(reps):
            if ts and time.perf_counter() - t_begin + max(ts) > budget_s:        # at least one timed repetition per leg
                break
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return ts

    for name, cfg_name, B, train in (("config3 kradar B=4 train", "kradar", 4, True),       # the headline leg first
                                     ("config3 kradar B=4 fwd", "kradar", 4, False),
                                     ("config2 kradar_radar_bev B=4 train", "kradar_radar_bev", 4, True),
                                     ("config1 kradar_camera_mono B=1 fwd (1280x720 frame)", "kradar_camera_mono", 1, False)):
        if legs and time.perf_counter() - t_begin > 0.8 * budget_s:
            legs[name] = {"ms": None, "samples_per_s": None, "timed_reps": 0, "skipped": "sample budget spent"}
            continue
        cfg = load_config(cfg_name)
        inputs = cfg["model"]["inputs"]
        sd = state(cfg)
        shapes = {"camera_mono": (720, 1280, 3)} if cfg_name == "kradar_camera_mono" else None   # un-resized frame
        batch = make_batch(inputs, B, seed=42, shapes=shapes) if shapes else make_batch(inputs, B, seed=42)
        labels = make_labels(B, seed=42)
        if train:
            params = [v for v in sd.values() if v.is_floating_point() and v.requires_grad]
            opt = torch.optim.AdamW(params, lr=cfg["train"]["optimizer"]["lr"])
            w = cfg["train"]["loss_weights"]

            def step():
                opt.zero_grad(set_to_none=True)
                out = O.dprt_forward(sd, cfg, batch, train=True)
                loss, _ = O.loss_forward(out, labels, w)
                loss.backward()
                opt.step()
            ts = timed(step, 1, 3)
        else:
            def fwd():
                with torch.no_grad():
                    O.dprt_forward(sd, cfg, batch, train=False)
            ts = timed(fwd, 2, 5)
        if ts:
            mean = sum(ts) / len(ts)
            legs[name] = {"ms": 1e3 * mean, "samples_per_s": B / mean, "timed_reps": len(ts)}
        else:
            legs[name] = {"ms": None, "samples_per_s": None, "timed_reps": 0}
    head = legs["config3 kradar B=4 train"]
    return {"value": head["samples_per_s"], "unit": "samples/s", "cores": cores, "kind": "port",
            "host_cores": os.cpu_count(), "cpu_model": cpu_model_name(),
            "sample": "BASELINE.md section 3 protocol on the torch-CPU fp32 oracle: configs 1-3, forward 2 warm-up + 5 timed, "
                      "train step (fwd + Hungarian set loss + bwd + AdamW) 1 warm-up + 3 timed; value = config 3 "
                      f"(kradar, batch 4) train samples/s; {cores} threads (fastest of a conv thread sweep on {host} host cores); "
                      f"bounded to ~{budget_s:.0f} s: legs cut short or skipped are marked; wall {time.perf_counter() - t_begin:.0f} s",
            "legs": legs}


def cpu_baseline_subprocess(args):
    """Run the CPU leg in a child process with a wall-clock bound so that the default bench finishes in minutes."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-only", "--cpu-threads", str(args.cpu_threads),
           "--cpu-timeout", str(args.cpu_timeout)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.cpu_timeout + 240,
                           env=dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES=""))
        for ln in reversed(r.stdout.strip().splitlines()):
            if ln.startswith("{"):
                return json.loads(ln)
        return {"value": None, "unit": "samples/s", "cores": None, "kind": "port", "sample": "failed: " + r.stderr[-300:]}
    except subprocess.TimeoutExpired:
        return {"value": None, "unit": "samples/s", "cores": None, "kind": "port",
                "sample": f"timed out after {args.cpu_timeout}s"}


SECONDARY_LEGS = {
    # BASELINE.json configs[1]: radar-only BEV backbone, batch 4, 1 GPU  |  configs[4]: bf16 mixed precision, its per-GPU share (batch 8)
    "radar_bev_b4": ["--config", "kradar_radar_bev", "--batch", "4"],
    "bf16_b8": ["--config", "kradar", "--dtype", "bf16", "--batch", "8"],
}


def secondary_legs(args):
    """Driver-clocked numbers for the configurations the headline line is not quoted on: each leg is this
    script again in a child process (`--leg`: the same trainer step, 5 warm-up + 12 timed steps, its own serialized-step
    conv roofline, 30 eval forwards), run AFTER and OUTSIDE the headline's timed region while this process idles."""
    import subprocess
    out = {}
    for name, flags in SECONDARY_LEGS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", "--full", "--steps", "12", "--warmup", "5", "--latency-reps", "30",
               "--no-cpu-baseline"] + flags
        t0 = time.perf_counter()
        try:
            env = {k: v for k, v in os.environ.items() if k != "DPFT_CONV_TABLE"}      # (the table is the headline step's)
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env)
            leg = None
            for ln in reversed(r.stdout.strip().splitlines()):
                if ln.startswith("{"):
                    leg = json.loads(ln)
                    break
            out[name] = leg if leg is not None else {"error": (r.stderr or "no output")[-300:]}
        except subprocess.TimeoutExpired:
            out[name] = {"error": "timed out after 240 s"}
        except Exception as e:      # a failed leg must not take the headline line with it
            out[name] = {"error": f"{type(e).__name__}: {e}"}
        out[name]["wall_s"] = round(time.perf_counter() - t0, 1)
        out[name]["cmd"] = "python bench.py " + " ".join(cmd[2:])
    return out


def exchange_diagnostics(trainer, bucket_trace, last_step_ms):
    """What a reader needs to judge the gradient exchange of an N > 1 run from the line alone: the collective library and its
    knobs, and for every bucket of the last timed step when its gradients were complete (`ready_ms`), when its collective started
    and ended (ms after the step's start on this rank).  A bucket whose `end_ms` is close to the step's end is exposed; gaps between
    one bucket's `end` and the next one's `start` that exceed `ready` spacing mean the exchange stream idles on dependencies."""
    try:
        ver = ".".join(str(v) for v in torch.cuda.nccl.version())
    except Exception:
        ver = None
    env = {k: v for k, v in os.environ.items() if k.startswith(("NCCL_", "RCCL_")) or k in ("HSA_ENABLE_IPC_MODE_LEGACY", "GPU_MAX_HW_QUEUES")}
    rows = sorted(bucket_trace or [], key=lambda r: r["start_ms"])
    total_mb = sum(r["mb"] for r in rows)
    busy = sum(r["end_ms"] - r["start_ms"] for r in rows)
    return {"library": "RCCL (torch.distributed backend 'nccl')", "rccl_version": ver, "env": env,
            "channels": os.environ.get("NCCL_MAX_NCHANNELS") or os.environ.get("NCCL_MIN_NCHANNELS") or
                        "library default (not exposed through torch; NCCL_DEBUG=INFO prints it at init)",
            "comm_stream": trainer.comm_placement, "collective_op": trainer.reducer.collective_op, "wire_dtype": trainer.comm_dtype,
            "buckets": len(rows), "exchanged_mb_per_step": round(total_mb, 1),
            "sum_of_collective_ms": round(busy, 3), "last_step_ms": last_step_ms,
            "first_ready_ms": rows[0]["ready_ms"] if rows else None, "last_end_ms": max((r["end_ms"] for r in rows), default=None),
            "bus_gb_per_s_while_busy": round(total_mb * 2 ** 20 / 1e9 / (busy * 1e-3), 1) if busy > 0 else None,
            "per_bucket": rows,
            "is": "rank 0, last timed step, ms after that step's first launch: ready = the bucket's last gradient written (firing "
                  "stream), start / end = its collective (a comm stream of our own: events around the call; the process group's own "
                  "stream: start = issue point, end = an event on a helper stream that waits for the work)"}


def runtime_state(trainer):
    """Fields the trainer settles while it runs (queue probe, host-pacing decision), read when the line is completed: at the end
    of the timed steps in a plain run, at the end of the run with --full."""
    return {
        "hardware_queues": {"distinct_besides_main": trainer.model.__dict__.get("_queues_found"),
                            "placement": os.environ.get("DPFT_STREAM_PLACEMENT", "probe"),
                            "note": "views and the camera's weight-gradient stream sit on probed, distinct hardware queues "
                                    "(dpft_stream_set); collectives: " + {"side": "in order on the camera's weight-gradient stream",
                                                                        "front": "in order on the last view's stream",
                                                                        "pg": "the process group's own stream",
                                                                        "own": "a dedicated stream"}.get(
                                        trainer.comm_placement, trainer.comm_placement)},
        "host_pacing": dict(mode=trainer.pace_host, **{k: v for k, v in trainer.__dict__.get("_pace_state", {}).items()
                                                       if k in ("decided", "host_ms", "gpu_ms")}),
    }


def decoder_runner(m, data):
    """-> (run, feats): ``run()`` = exactly one dpft_decoder_forward_f32 call (the fused inference decoder of one
    IMPFusion.forward) on the encoded pyramids of ``data``.  Also used by tools/decoder_only.py for the PMC passes."""
    m.eval()
    with torch.no_grad():
        feats = m._encode_views(data)
        proj = m._get_projetions(m.inputs, data)
        shp = [data[f"{i}_shape"][:, :2] for i in m.inputs]
        flags = None                                   # transformation.any() evaluated on the device, as in DPRT.forward
        c0 = m.querent(data)
        vb = [feats[i] for i in m.inputs]
        m.fuser(batch=vb, shape=shp, projection=proj, out=c0, has_transformation=flags)   # builds the fused decoder
        fd = m.fuser.__dict__.get("_fused_decoder")
        if not fd:
            raise RuntimeError("the fused HIP decoder is not active for this configuration")
        fd.prepare(vb, shp, proj, c0, flags)
    return fd.launch, feats


DUMP_PARAM_SAMPLES = 1 << 22        # 16 MiB of float32 parameter values


def dump_outputs(out_dir, loss, losses, model):
    """What the last timed step computed, as ``out_dir/<name>.npy``: ``train_step``'s return values -- ``loss.npy`` and
    ``loss_<term>.npy`` for every term of the set loss, float64 -- and ``params_sample.npy``, the parameters AdamW wrote in
    that step, float32: a fixed sample of up to 2^22 positions of the flat concatenation of ``model.parameters()`` (logical
    layout, registration order), drawn from numpy's ``default_rng(0)`` and sorted.  The inputs are seeded, so two builds
    run with the same arguments can be compared file for file -- with a tolerance: the fp32 atomics of the training decoder's
    backward make the trajectory differ from run to run (two runs of 5 + 20 steps on one MI355X: loss terms up to 3.5e-3
    relative, parameters within 9e-4 of the largest magnitude and 1e-2 relative L2), and the spread grows with the number of
    steps."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "loss.npy"), loss.detach().double().cpu().numpy())
    for k, v in losses.items():
        np.save(os.path.join(out_dir, f"loss_{k}.npy"), torch.as_tensor(v).detach().double().cpu().numpy())
    params = list(model.parameters())
    offs = np.concatenate(([0], np.cumsum([p.numel() for p in params])))
    idx = np.unique(np.random.default_rng(0).integers(0, int(offs[-1]), size=min(DUMP_PARAM_SAMPLES, int(offs[-1]))))
    chunks = []
    for p, start, lo, hi in zip(params, offs[:-1], np.searchsorted(idx, offs[:-1]), np.searchsorted(idx, offs[1:])):
        if hi > lo:
            sel = torch.from_numpy(idx[lo:hi] - start).to(p.device)
            chunks.append(p.detach().reshape(-1)[sel].float().cpu())
    np.save(os.path.join(out_dir, "params_sample.npy"), torch.cat(chunks).numpy())


def main():
    args = parse()
    if args.cpu_baseline_only:
        print(json.dumps(cpu_baseline(args.cpu_threads, float(args.cpu_timeout))))
        return
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: dpft_amd has no CPU path")
    # test hook (tests/test_gpu_distributed.py): all ranks on ONE device over gloo -- RCCL refuses two ranks per GPU
    one_device = os.environ.get("DPFT_BENCH_ONE_DEVICE_GLOO") == "1"
    if one_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if one_device:
            dist.init_process_group(backend="gloo")
        else:
            dist.init_process_group(backend="nccl", device_id=device)
    elif args.force_collectives:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        dist.init_process_group(backend="nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=device)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    collective = world > 1 or args.force_collectives

    from dpft_amd.configs import load_config
    from dpft_amd.hip import ops
    from dpft_amd.models import build
    from dpft_amd.synthetic import make_batch, make_labels
    from dpft_amd.training.trainer import DataParallelTrainer

    cfg = load_config(args.config)
    if args.dtype == "bf16":
        cfg["computing"]["conv_compute"] = "bf16"
    elif args.dtype == "f32x3":      # experimental: fp32 operands as three bf16 terms on the bf16 matrix cores
        cfg["computing"]["conv_compute"] = "bf16x3"
    torch.manual_seed(cfg["computing"]["seed"])
    model = build("dprt", cfg)
    if args.no_split:
        ops.conv_set_split(False)
    trainer = DataParallelTrainer(model, cfg, device, bucket_mb=args.bucket_mb, comm_dtype=args.comm_dtype,
                                  force_collectives=args.force_collectives)
    inputs = cfg["model"]["inputs"]
    B = args.batch
    # weak scaling: every rank owns its own seeded shard of the global batch, resident in HBM
    data = make_batch(inputs, B, seed=cfg["computing"]["seed"] + rank, device=device)
    labels = make_labels(B, seed=cfg["computing"]["seed"] + rank, device=device)

    def sync():
        if collective:
            dist.barrier()
        torch.cuda.synchronize()

    if not args.no_graphs:
        try:
            trainer.enable_graphs(data)
        except Exception as e:          # keep the measurement valid (same work, eager launches) rather than abort the rank
            print(f"[bench] rank {rank}: decoder graph capture failed ({type(e).__name__}: {e}); running ungraphed",
                  file=sys.stderr, flush=True)
            torch.cuda.synchronize()
            trainer.model.disable_fuser_graph()
    # set-up, like enable_graphs() above: the encoders' launch plans capture their hipGraphs on the third call (two eager
    # executions first) -- with fewer than three warm-up steps that capture would fall into the timed region
    for _ in range(max(0, 3 - args.warmup)):
        trainer.train_step(data, labels)
    for _ in range(args.warmup):
        trainer.train_step(data, labels)
    sync()
    # per-step spread: one event per step boundary on the main stream (no sync inside the timed region -- the events
    # cost ~1 us of queue time each); a step's figure is the GPU time between two consecutive boundaries
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(args.steps):
        if collective and i == args.steps - 1:
            trainer.reducer.trace_begin()      # per-bucket ready / start / end marks of the LAST timed step (~3 event records per bucket)
        loss, losses = trainer.train_step(data, labels)
        marks[i + 1].record()
    sync()
    elapsed = time.perf_counter() - t0
    bucket_trace = trainer.reducer.trace_report() if collective else None
    step_ms_order = [marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps)]
    step_ms = sorted(step_ms_order)
    # None at one rank without forced collectives: there is no exchange to expose (0.0 would read like a measurement)
    exposed_ms = trainer.reducer.exposed_ms() if collective else None
    if collective:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    ms_per_step = 1e3 * elapsed / args.steps
    value = world * B * args.steps / elapsed
    line = None
    if rank == 0:
        line = {
            "metric": f"training samples/sec (K-Radar C+R, bs{B}/GPU)", "value": value, "unit": "samples/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
            "step_ms_first8": [round(v, 2) for v in step_ms_order[:8]],      # (in order: the steps right behind the sync at the start)
            "step_ms_min": step_ms[0], "step_ms_median": step_ms[len(step_ms) // 2], "step_ms_max": step_ms[-1],
            "step_ms_is": "rank 0, per step: HIP events on the main stream at every step boundary of the timed region",
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": f"{args.config}.json full C+R dual-perspective fusion train step, batch {B}/GPU "
                                   "(camera 512x910x3 ResNet-101, radar BEV 256x107x6 + front 37x107x6 ResNet-50, "
                                   "FPN->16ch, IMPFusion 4 it x 3 views, Hungarian set loss, AdamW)",
                       "global_batch": world * B, "parallelism": f"dp{world}",
                       "precision": {"f32": "fp32 (reference arithmetic; fp32 tensors and fp32 results everywhere)" +
                                            ("" if args.no_split else ": the big multi-tap conv GEMMs form each fp32 product from six exact bf16 "
                                             "term products on the bf16 matrix cores (3 x bf16 split, fp32 accumulation), the rest runs on "
                                             "the fp32 MFMA"),
                                     "bf16": "mixed (BASELINE.json configs[4]): bf16 operands / fp32 accumulation in the conv GEMMs; "
                                             "activations of the large (camera) encoder bodies stored as bf16 in HBM, BatchNorm "
                                             "statistics / accumulators / master weights / decoder / loss / AdamW fp32",
                                     "f32x3": "experimental: fp32 conv operands as three bf16 terms, six term products "
                                              "on the bf16 matrix cores, fp32 accumulation"}[args.dtype]},
            "step_definition": "zero_grad, forward, Hungarian set loss, backward, bucketed all-reduce, AdamW; the per-step "
                               "eval_fn of the reference's loop (trainer.py:134-136) is not part of the timed step",
            "rccl_ranks": world, "collectives_forced": bool(args.force_collectives and world == 1),
            "collective_op": (trainer.reducer.collective_op + (" (one rank: avg == sum; RCCL's one-rank AVG is a pre-multiply pass "
                              "over every bucket, +0.8 ms/step, DPFT_COLLECTIVE_OP=avg)" if world == 1 else ""))
                             if trainer.collective else None,
            "exposed_allreduce_ms": exposed_ms,
            "exposed_allreduce_is": "last timed step: from the point the rank's CURRENT (main) stream has finished its own "
                                    "backward work to the completion of the last bucket's collective, bracketed by events on "
                                    "that stream; collectives of view-stream buckets that finish earlier are not in it",
            "dp_bucket_mb": trainer.bucket_mb,
            "dp_exchange": exchange_diagnostics(trainer, bucket_trace, step_ms_order[-1] if step_ms_order else None) if collective else None,
            "dp_comm_dtype": trainer.comm_dtype,
            "loss": float(loss),
            **runtime_state(trainer),
            "host_pacing_is": "DataParallelTrainer._pace: the host waits for the GPU to reach the decoder's forward graph before it enqueues "
                              "the backward; 'auto' does so when four measured steps say the host's own period is < 0.8 x the GPU's",
            "full": bool(args.full),
            "full_is": "--full adds the conv and decoder rooflines, the loss window, eval-forward latency, the CPU baseline and the "
                       "secondary legs, all measured after the timed steps",
        }
        if args.dump_outputs:           # before anything else runs a step: the values of the LAST timed step
            dump_outputs(args.dump_outputs, loss, losses, trainer.model)
    if not args.full:
        if rank == 0:
            print(json.dumps(line))
        if collective:
            dist.barrier()
            dist.destroy_process_group()
        return

    # ---- roofline of the dominant kernel family: fp32 MFMA implicit-GEMM convolutions --------------
    roof, per_kind = None, {}
    # one serialized step (no concurrent view streams, no side-stream weight gradients): every conv launch is
    # bracketed by HIP events and runs alone, so its duration is the kernel's, not its share of a busy device.
    # EVERY rank takes the step (it contains the gradient all-reduce); only rank 0 records.
    torch.cuda.synchronize()
    trainer.model.concurrent_views = False
    if rank == 0:
        ops.profile_start()
    trainer.train_step(data, labels)
    recs = ops.profile_collect() if rank == 0 else []
    trainer.model.concurrent_views = True
    if rank == 0:
        tot_f, tot_t = 0.0, 0.0
        shapes = {}
        fam_f, fam_t, fam_n = {}, {}, {}      # per kernel family, as tagged by the library's dispatch code at the launch
        shape_fam = {}
        for kind, flops, dt, shape, fam in recs:
            sh = shapes.setdefault((kind,) + shape, [0.0, 0.0, 0])
            sh[0] += flops; sh[1] += dt; sh[2] += 1
            shape_fam[(kind,) + shape] = fam
            fam_f[fam] = fam_f.get(fam, 0.0) + flops
            fam_t[fam] = fam_t.get(fam, 0.0) + dt
            fam_n[fam] = fam_n.get(fam, 0) + 1
            k = per_kind.setdefault(kind, [0.0, 0.0, 0])
            k[0] += flops; k[1] += dt; k[2] += 1
            tot_f += flops; tot_t += dt
        if os.environ.get("DPFT_CONV_TABLE"):
            with open(os.environ["DPFT_CONV_TABLE"], "w") as f:
                f.write("kind B H W C K k s calls total_us TFLOPs family\n")
                for key, v in sorted(shapes.items(), key=lambda kv: -kv[1][1]):
                    f.write(" ".join(str(x) for x in key) + f" {v[2]} {v[1] * 1e6:.1f} {v[0] / v[1] / 1e12:.1f} {shape_fam[key]}\n")
            # algorithmic flops per kernel family of this step (what tools/roofline_from_rocprof.py --families prices the
            # committed kernel-trace summary with: time per family from the kernel names, flops from here)
            with open(os.path.splitext(os.environ["DPFT_CONV_TABLE"])[0] + "_families.json", "w") as f:
                json.dump({"gflop_per_step": {k: v / 1e9 for k, v in fam_f.items()}, "launches_per_step": fam_n,
                           "batch": B, "dtype": args.dtype, "config": args.config,
                           "source": "bench.py: dpft_profile_get_family tags of one serialized step"}, f, indent=1)
        n_launch = sum(k[2] for k in per_kind.values())
        # algorithmic HBM bytes of the same calls: every conv call (fwd / dgrad / wgrad alike) touches its input map, its
        # output map and its weights once -- x + y + w fp32 elements (shape key = kind, B, H, W, C, K, k, s; H x W = the
        # conv's INPUT map, output = ceil(H / s) x ceil(W / s) with "same" padding)
        alg_bytes = 0.0
        for key, v in shapes.items():
            _, b_, h_, w_, c_, k_, ks_, st_ = key
            oh, ow = -(-h_ // st_), -(-w_ // st_)
            alg_bytes += v[2] * 4.0 * (b_ * h_ * w_ * c_ + b_ * oh * ow * k_ + k_ * c_ * ks_ * ks_)
        # two more views of the same launch log: FLOP-weighted mean of the per-shape rates (SURVEY 8d wording), and
        # the camera encoder alone (94 % of the FLOPs; the radar encoders' tiny GEMMs are launch-bound and, in the
        # real step, hidden behind the camera on their own streams -- in this serialized step they count in full)
        cam_w = {910, 455, 228, 114, 57, 29}          # widths of the camera feature maps (input of the conv)
        cam = [v for key, v in shapes.items() if key[3] in cam_w]
        cam_f, cam_t = sum(v[0] for v in cam), sum(v[1] for v in cam)
        # HBM bytes per conv LAUNCH from the committed PMC passes of this round (tools/r06_profile.sh: FETCH_SIZE and
        # WRITE_SIZE in separate rocprofv3 runs, FETCH_SIZE doubled per the gfx950 note of MI355X_MICROARCH.md).  It is a
        # constant read from profiles/, not a measurement of this run: the file is named in the line.
        traffic, traffic_src = None, None
        prof_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
        for name in ("r06_conv_traffic_pmc.json", "r05_conv_traffic_pmc.json", "r04_conv_traffic_pmc.json", "r03_conv_traffic_pmc.json"):
            if os.path.exists(os.path.join(prof_dir, name)):
                with open(os.path.join(prof_dir, name)) as f:
                    traffic = json.load(f).get("traffic_bytes_per_launch")
                traffic_src = "profiles/" + name
                break
        # mixed precision: priced against the dense bf16 MFMA peak (2.5 PF) -- the kernels are then bound by their operand
        # path (global loads -> LDS -> fragments, two barriers per 64-deep K-step), not by the matrix pipe
        peak = PEAK_BF16_MFMA_TFLOPS if args.dtype == "bf16" else PEAK_F32_MFMA_TFLOPS
        split = args.dtype == "f32" and ops.conv_get_split()
        # share of the conv flops that ran as split products: what the library's dispatch tagged 'x3' at the launch (forward,
        # data gradient AND weight gradient kernels of conv_x3.hip) -- not a shape predicate
        split_f = fam_f.get("x3", 0.0)
        # pipe-correct pricing: every launch against the peak of the pipe that ran it -- fp32 MFMA 157.3 TF,
        # six-product split 2500 / 6 = 416.7 TF, bf16 operands 2500 TF, vector-ALU kernels 157.3 TF (fp32 FMA rate)
        fam_peak = {"f32": PEAK_F32_MFMA_TFLOPS, "x3": PEAK_BF16_MFMA_TFLOPS / 6.0, "bf16": PEAK_BF16_MFMA_TFLOPS, "vector": PEAK_F32_MFMA_TFLOPS}
        ideal_s = sum(fam_f[k] / (fam_peak[k] * 1e12) for k in fam_f)
        family = {"f32": "fp32 MFMA (v_mfma_f32_32x32x2_f32)" + ("; multi-tap filters >= 2 GFLOP: 3 x bf16 split, six v_mfma_f32_32x32x16_bf16 "
                         "term products per fp32 product, fp32 accumulation (conv_x3.hip)" if split else ""), "bf16": "bf16 MFMA (v_mfma_f32_32x32x16_bf16, fp32 accumulation)",
                  "f32x3": "3 x bf16 split products on the bf16 MFMA, fp32 accumulation"}[args.dtype]
        # (round 3: the data-gradient launches also carry the BatchNorm-backward reduction of the layer they feed; its
        # time is inside their brackets although it is not conv work)
        # Accounting.  A bracket spans everything one dpft_conv2d_nhwc_* call launches: the implicit-GEMM
        # main loop AND the split-K / slab reduction kernels it needs.  `frac` uses the RAW bracket time.  rocprofv3's
        # kernel durations of the same serialized step (profiles/r03_serialized_step_kernel_stats.csv, recomputed by
        # tools/roofline_from_rocprof.py) give the same number within a few %; `frac_main_kernels_only` removes the
        # reduction kernels and the ~4.5 us an empty event bracket costs, i.e. what round 1 reported as `frac`.
        ovh = float(ops.lib.dpft_profile_overhead_ms()) * 1e-3
        raw_t = tot_t + ovh * n_launch
        # committed rocprofv3 summaries of this step (newest round first): the serialized one the line must agree with, and the
        # plain (concurrent-stream) one that gives the conv kernels' durations inside the real step
        rnd = next((r for r in ("r06", "r05") if os.path.exists(os.path.join(prof_dir, r + "_serialized_step_kernel_stats.csv"))), "r05")
        in_step = {}
        try:
            with open(os.path.join(prof_dir, rnd + "_roofline_from_rocprof_plain_steps.json")) as f:
                in_step = json.load(f)
        except Exception:
            in_step = {}
        roof = {"bound": "mfma", "achieved": tot_f / raw_t / 1e12, "peak": peak, "unit": "TFLOP/s",
                "frac": tot_f / raw_t / 1e12 / peak,
                "traffic": traffic if args.dtype == "f32" else None, "traffic_is": "HBM bytes per conv launch", "traffic_source": traffic_src,
                "algorithmic_bytes_per_launch": alg_bytes / max(n_launch, 1),
                "algorithmic_bytes_is": "x + y + w fp32 elements of every conv call (input map, output map, weights once each), "
                                        "mean over the step's conv calls",
                "traffic_over_algorithmic": (traffic * n_launch / alg_bytes) if (traffic and args.dtype == "f32" and alg_bytes) else None,
                "kernel": f"igemm_pipe/wgrad_pipe/igemm_gen ({family} implicit-GEMM conv family, incl. their split-K reductions "
                          "and the BatchNorm-backward reductions fused into the data-gradient epilogues)",
                "launches_per_step": n_launch, "avg_launch_us": 1e6 * raw_t / max(n_launch, 1),
                "conv_ms_per_step": 1e3 * raw_t, "algorithmic_gflop_per_step": tot_f / 1e9,
                "timing": "HIP events around every conv call of one serialized step, on the launch stream (raw bracket time)",
                "frac_main_kernels_only": tot_f / tot_t / 1e12 / peak,
                "event_bracket_overhead_us": 1e6 * ovh,
                "rocprof_summary": (f"profiles/{rnd}_serialized_step_kernel_stats.csv (tools/roofline_from_rocprof.py -> "
                                    f"profiles/{rnd}_roofline_from_rocprof.json)" if args.dtype == "f32" and B == 4 else None),
                "frac_in_step": in_step.get("frac") if args.dtype == "f32" and B == 4 else None,
                "frac_in_step_source": (f"profiles/{rnd}_roofline_from_rocprof_plain_steps.json <- {rnd}_train_step_kernel_stats.csv (rocprofv3 "
                                        "--kernel-trace --stats over plain, un-serialized steps; a constant of the committed profile, "
                                        "not of this run)") if in_step else None,
                "precision": ("fp32 (3 x bf16 split, 6 products) on the multi-tap conv GEMMs >= 2 GFLOP, fp32 MFMA elsewhere: fp32 tensors "
                              "in and out, error vs fp64 below the fp32 MFMA path's on every conv of the step "
                              "(tests/test_gpu_conv_table.py)" if split else
                              {"f32": "fp32 MFMA", "bf16": "bf16 operands, fp32 accumulation", "f32x3": "3 x bf16 split"}[args.dtype]),
                "split_share_of_conv_flops": (split_f / tot_f) if tot_f > 0 else None,
                "split_share_is": "flops of the launches the library's dispatch code tagged as conv_x3.hip kernels (igemm_x3 forward / data "
                                  "gradient AND wgrad_x3) / all conv flops (dpft_profile_get_family; not a shape predicate)",
                "split_peak_tflops": PEAK_BF16_MFMA_TFLOPS / 6.0,
                "frac_blended": ideal_s / raw_t if raw_t > 0 else None,
                "frac_blended_is": "sum_i(flops_i / peak_i) / conv time of the serialized step, peak_i of the pipe that ran launch i: "
                                   "fp32 MFMA 157.3 TF | six-product bf16 split 416.7 TF | bf16 operands 2500 TF | vector-ALU kernels 157.3 TF",
                "by_family": {k: {"gflop_per_step": fam_f[k] / 1e9, "ms_per_step": 1e3 * (fam_t[k] + ovh * fam_n[k]), "launches": fam_n[k],
                                  "tflops": fam_f[k] / (fam_t[k] + ovh * fam_n[k]) / 1e12, "peak_tflops": fam_peak[k],
                                  "frac_of_own_peak": fam_f[k] / (fam_t[k] + ovh * fam_n[k]) / 1e12 / fam_peak[k]} for k in sorted(fam_f)},
                "frac_note": "frac prices ALL conv flops of the step against the fp32 MFMA peak (157.3 TF), whichever pipe ran them; "
                             "frac_blended prices every launch against its own pipe (by_family); frac_in_step is the same ratio as "
                             "frac with the conv kernels' durations INSIDE the real, un-serialized step (they share CUs with the other "
                             "streams there), from the committed kernel trace",
                "peak_note": "157.3 TF = 2.4 GHz nominal; under sustained fp32 MFMA load the chip clocks ~2.16 GHz "
                             "(64-cycle MFMA measured at 71 nominal cycles, tools/probes/mfma_valu_overlap.hip), i.e. ~142 TF "
                             "is what the matrix pipe delivers; frac is priced against the nominal peak",
                "per_kind_tflops": {k: v[0] / (v[1] + ovh * v[2]) / 1e12 for k, v in per_kind.items()},
                "conv_frac_camera_only": (cam_f / cam_t / 1e12 / peak) if cam_t > 0 else None,
                "camera_encoder_share_of_conv_time": (cam_t / tot_t) if tot_t > 0 else None}

    if args.leg:      # child of secondary_legs(): one compact line, nothing else
        fwd_mean, fwd_std = trainer.inference_time(data, warmup=5, reps=args.latency_reps)
        if rank == 0:
            print(json.dumps({
                "samples_per_s": value, "ms": ms_per_step, "step_ms_median": step_ms[len(step_ms) // 2], "steps": args.steps,
                "batch": B, "dtype": args.dtype, "config": args.config, "fwd_ms_per_frame": fwd_mean / B,
                "frac": roof["frac"] if roof else None, "peak_tflops": roof["peak"] if roof else None,
                "frac_blended": roof["frac_blended"] if roof else None,
                "conv_ms_per_step": roof["conv_ms_per_step"] if roof else None,
                "conv_gflop_per_step": roof["algorithmic_gflop_per_step"] if roof else None, "loss": float(loss)}))
        return
    # ---- the step's host window: GPU time between the matcher's cost kernel and the start of the decoder's backward graph ------
    # (the one place where the GPU waits for the host: read-back of the cost matrices, assignments, upload, criterion + gradient
    # launches, graph launch).  Events recorded by wrapping the two call sites; median over 12 extra steps after the timed region.
    loss_window_us = None
    g_ = trainer.model.__dict__.get("_graphed_fuser")
    if rank == 0 and world == 1 and not collective and g_ is not None and hasattr(trainer.loss_fn, "_to_host"):      # (one rank: the
        # extra steps hold no collective another rank would have to join)
        n_w = 12
        ev_c = [torch.cuda.Event(enable_timing=True) for _ in range(n_w)]
        ev_b = [torch.cuda.Event(enable_timing=True) for _ in range(n_w)]
        cur = [0]
        o_replay = g_.bwd_graph.replay

        def _replay():
            ev_b[cur[0]].record()
            return o_replay()
        trainer.loss_fn.__dict__["_cost_hook"] = lambda: ev_c[cur[0]].record()
        g_.bwd_graph.replay = _replay
        try:
            for i in range(n_w):
                cur[0] = i
                trainer.train_step(data, labels)
            torch.cuda.synchronize()
            w = sorted(ev_c[i].elapsed_time(ev_b[i]) * 1e3 for i in range(n_w))
            loss_window_us = w[n_w // 2]
        except Exception:
            loss_window_us = None
        finally:
            trainer.loss_fn.__dict__.pop("_cost_hook", None)
            g_.bwd_graph.replay = o_replay
    # ---- fwd ms/frame with the reference's latency protocol (evaluator.py:109-125) ----------------
    fwd_mean, fwd_std = trainer.inference_time(data, warmup=10, reps=args.latency_reps)
    # single-frame latency (what a "low inference time" claim is about, README.md:16 of the reference; its own protocol
    # times a batch): the same protocol on batch 1
    data1 = {k: v[:1].contiguous() for k, v in data.items()}
    fwd1_mean, fwd1_std = trainer.inference_time(data1, warmup=10, reps=max(20, args.latency_reps // 3))

    # ---- HBM roofline of the deformable fusion decoder (SURVEY 8d "Roofline B") -------------------------
    # unit of work = one IMPFusion.forward (eval); algorithmic bytes = every cross-attention call streams its
    # view's 16-channel fp32 pyramid once + query-side I/O + parameters
    dec = dec_train = None
    if rank == 0:
        m = trainer.model
        with torch.no_grad():
            run, feats = decoder_runner(m, data)
            for _ in range(5):
                run()
            reps = max(args.latency_reps, 20)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                run()
            e1.record()
            torch.cuda.synchronize()
        t_dec = e0.elapsed_time(e1) * 1e-3 / reps
        tokens = sum(int(l.shape[1] * l.shape[2]) for i in m.inputs for l in feats[i].values())
        fcfg = cfg["model"]["fuser"]
        n_calls = fcfg["i_iter"] * len(m.inputs)
        dec_bytes = fcfg["i_iter"] * B * tokens * 64 + n_calls * B * fcfg["n_queries"] * (16 + 16 + 2 + 16) * 4 + 0.42e6
        # counter traffic of the decoder kernels (tools/r06_profile.sh: FETCH_SIZE x 2 + WRITE_SIZE per forward, committed)
        dec_traffic, dec_src = None, None
        for pname in ("r05_decoder_traffic_pmc.json", "r04_decoder_traffic_pmc.json", "r03_decoder_traffic_pmc.json"):
            pmc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", pname)
            if os.path.exists(pmc):
                with open(pmc) as f:
                    dec_traffic = json.load(f).get("traffic_bytes_per_forward")
                dec_src = "profiles/" + pname
                break
        dec = {"bound": "hbm", "achieved": dec_bytes / t_dec / 1e9, "peak": 8000.0, "unit": "GB/s",
               "frac": dec_bytes / t_dec / 8.0e12, "traffic": dec_traffic, "traffic_is": "HBM bytes per forward (counters)",
               "traffic_source": dec_src, "decoder_fwd_us": t_dec * 1e6,
               "algorithmic_mb": dec_bytes / 1e6, "kernel": "decoder_scores_head + decoder_xattn "
               f"({2 * fcfg['i_iter'] - 1} launches per forward: iteration 0's self-attention output, a constant of the "
               "weights, is made when the weights are packed; the last iteration's heads ride in its cross-attention launch)",
               "note": "frac prices the measured time against the time 8 TB/s needs for the ALGORITHMIC bytes of SURVEY 8d "
                       "(every cross-attention call streaming its pyramid once); the sample-then-project kernels touch far "
                       "fewer HBM bytes (traffic), they are bound by L2 line requests and kernel-boundary latency",
               "timing": f"{reps} back-to-back dpft_decoder_forward_f32 calls between two HIP events on the launch stream"}
        # second accounting: the SUM of the decoder kernels' durations per forward in the committed rocprofv3
        # summary (tools/roofline_from_rocprof.py --decoder) -- a constant read from profiles/, named in the line
        for pname in ("r05_decoder_roofline_from_rocprof.json", "r04_decoder_roofline_from_rocprof.json"):
            pj = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", pname)
            if os.path.exists(pj) and args.dtype == "f32" and B == 4:
                with open(pj) as f:
                    rj = json.load(f)
                dec["rocprof_kernel_sum_us"] = rj.get("kernel_sum_us_per_forward")
                dec["frac_rocprof_kernel_sum"] = rj.get("frac")
                dec["rocprof_summary"] = "profiles/" + pname + " <- " + str(rj.get("source"))
                break
        # ---- training decoder (forward + backward graphs of the fusion decoder, SURVEY 8d "Backward") ----------------
        # unit = one IMPFusion forward + backward at B: bytes_fwd + bytes_bwd, bytes_bwd = bytes_fwd + the gradient
        # pyramids written once.  Timed as `reps` replays of the trainer's captured forward and backward graphs
        # back to back (everything the decoder section of a step launches: fused blocks, rows_outer, pack kernels and
        # the few ATen nodes left), between two HIP events.  The backward ACCUMULATES into the pyramid-gradient buffers
        # and the gradient buckets: the values are garbage afterwards, which is why this runs after the timed region.
        dec_train = None
        g = trainer.model.__dict__.get("_graphed_fuser")
        if g is not None:
            bwd_bytes = dec_bytes + B * tokens * 64
            for _ in range(3):
                g.fwd_graph.replay(); g.bwd_graph.replay()
            torch.cuda.synchronize()
            tr_reps = max(20, min(reps, 100))
            e0.record()
            for _ in range(tr_reps):
                g.fwd_graph.replay()
                g.bwd_graph.replay()
            e1.record()
            torch.cuda.synchronize()
            t_tr = e0.elapsed_time(e1) * 1e-3 / tr_reps
            e0.record()
            for _ in range(tr_reps):
                g.fwd_graph.replay()
            e1.record()
            torch.cuda.synchronize()
            t_trf = e0.elapsed_time(e1) * 1e-3 / tr_reps
            dec_train = {"bound": "hbm", "achieved": (dec_bytes + bwd_bytes) / t_tr / 1e9, "peak": 8000.0, "unit": "GB/s",
                         "frac": (dec_bytes + bwd_bytes) / t_tr / 8.0e12, "traffic": None,
                         "algorithmic_mb": (dec_bytes + bwd_bytes) / 1e6, "decoder_train_fwd_bwd_us": t_tr * 1e6,
                         "decoder_train_fwd_us": t_trf * 1e6, "decoder_train_bwd_us": (t_tr - t_trf) * 1e6,
                         "kernel": "sa_train_* + xf_train_* + hd_train_* + rows_outer + pack kernels (the decoder's forward "
                                   "and backward hipGraphs, dropout on)",
                         "timing": f"{tr_reps} replays of the captured forward + backward graphs between two HIP events"}

    if rank == 0 and roof is not None:      # the other kernels' fractions inside the record the driver parses
        if dec is not None:
            roof["decoder_frac"] = dec["frac"]
            roof["decoder_kernel_sum_frac"] = dec.get("frac_rocprof_kernel_sum")
            roof["decoder_fwd_us"] = dec["decoder_fwd_us"]
        if dec_train is not None:
            roof["decoder_train_frac"] = dec_train["frac"]
            roof["decoder_train_fwd_bwd_us"] = dec_train["decoder_train_fwd_bwd_us"]
    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline_subprocess(args)
    secondary = None
    # (--no-cpu-baseline is what the A/B scripts under tools/ pass for a quick line: no child processes at all then)
    if rank == 0 and world == 1 and not collective and not args.no_secondary and not args.no_cpu_baseline and args.config == "kradar" and args.dtype == "f32":
        torch.cuda.synchronize()
        secondary = secondary_legs(args)

    if rank == 0:
        line.update(runtime_state(trainer))
        line.update({
            "fwd_ms_per_frame": fwd_mean / B, "fwd_ms_per_batch": fwd_mean, "fwd_ms_std": fwd_std,
            "fwd_ms_batch1": fwd1_mean, "fwd_ms_batch1_std": fwd1_std,
            "fwd_protocol": f"10 warm-up + {args.latency_reps} event-timed eval forwards of one batch (evaluator.py:109-125)",
            "loss_window_us": loss_window_us,
            "loss_window_is": "median GPU time from the end of the matcher's cost kernel to the start of the decoder's backward graph "
                              "(assignment kernel -- one wavefront per sample, no host round trip --, criterion + gradient kernels; "
                              "DPFT_LSAP_DEV=0: read-back, host assignments, upload instead), 12 steps after the timed region",
            "loss_window_assignments": "device" if getattr(trainer.loss_fn, "assign_on_device", False)
                                       and os.environ.get("DPFT_LSAP_DEV", "1") != "0" else "host",
            "roofline": roof, "roofline_decoder": dec, "roofline_decoder_train": dec_train, "cpu_baseline": cpu,
            "secondary": secondary,
            "secondary_is": "BASELINE.json configs[1] (kradar_radar_bev.json, batch 4) and configs[4]'s per-GPU share (kradar.json, bf16 "
                            "mixed precision, batch 8): this script as a child process per leg, after and outside the headline's timed "
                            "region -- 5 warm-up + 12 timed steps, barrier + device sync on both sides; frac = that leg's conv family "
                            "against its own peak (fp32 MFMA 157.3 TF | bf16 2500 TF), serialized-step event brackets",
        })
        print(json.dumps(line))
    if collective:
        dist.barrier()                    # rank 0 is still measuring (decoder roofline) when the others get here
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
