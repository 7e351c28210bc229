"""Times the multi-scale deformable attention operator at the shape the Deformable-DETR family runs it at (DESIGN.md section 3,
"Typed MSDA operator"): N = 2, M = 8 heads x D = 32 channels, P = 4 points, four levels (100,134) (50,67) (25,34) (13,17)
(S = 17 821 pixels), with Lq = S (the encoder form) and Lq = 300 (the decoder form), forward and backward, through

  f32      dpft_msda_fwd_f32 / dpft_msda_bwd_f32 (msda.hip; the backward timed WITH the zero fill of grad_value its contract asks
           the caller for -- the typed entry clears its sums itself, so both columns are the whole cost of a backward)
  typed0   dpft_msda_fwd_typed / dpft_msda_bwd_typed with dtype 0 (fp32 storage)
  typed1   ... dtype 1 (IEEE half), fp32 locations
  typed2   ... dtype 2 (bf16), fp32 locations

Every call is a raw C-ABI call on preallocated tensors between device events; per variant 5 warm-up calls, then --reps timed
calls per block, --blocks blocks with the variants alternating inside a block; median and minimum over all timed calls.  Beside
each backward: the atomic floor = bytes the grad_value sums take as fp32 atomics (N Lq M L P x 4 corners x D x 4 bytes) over the
chip-wide float-atomic rate of 1.3 TB/s, and the ratio of the measured time to it.  Before timing, the typed results are compared
with the f32 kernels' on the same inputs (largest absolute difference, printed).
Usage: python tools/msda_bench.py [--reps 20] [--blocks 3] [--out profiles/msda_typed.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dpft_amd.hip.lib import lib, ptr, stream      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--blocks", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msda_typed.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "msda_bench.py measures on the GPU; there is nothing to measure without one"
assert args.reps * args.blocks >= 20

DEV = torch.device("cuda", 0)
N, M, D, P = 2, 8, 32, 4
SHAPES = [(100, 134), (50, 67), (25, 34), (13, 17)]
L, S = len(SHAPES), sum(h * w for h, w in SHAPES)
ATOMIC_RATE = 1.3e12
TYPES = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def make_case(Lq):
    g = torch.Generator().manual_seed(7 + Lq)
    c = {"Lq": Lq,
         "value": torch.randn(N, S, M, D, generator=g).to(DEV),
         "loc": (torch.rand(N, Lq, M, L, P, 2, generator=g) * 1.1 - 0.05).to(DEV),      # a few samples fall off the maps
         "attn": torch.softmax(torch.randn(N, Lq, M, L * P, generator=g), -1).view(N, Lq, M, L, P).to(DEV),
         "go": torch.randn(N, Lq, M * D, generator=g).to(DEV),
         "shapes": torch.tensor(SHAPES, dtype=torch.int64, device=DEV),
         "lsi": torch.tensor([0] + [int(v) for v in torch.tensor([h * w for h, w in SHAPES]).cumsum(0)[:-1]], dtype=torch.int64,
                             device=DEV)}
    return c


def variant(c, name):
    """-> (fwd(), bwd(), tensors) closures over preallocated buffers."""
    Lq = c["Lq"]
    dtype = {"f32": 0, "typed0": 0, "typed1": 1, "typed2": 2}[name]
    T = TYPES[dtype]
    v, a, go = c["value"].to(T), c["attn"].to(T), c["go"].to(T)
    loc = c["loc"]
    out, gv, ga, gl = torch.empty(N, Lq, M * D, dtype=T, device=DEV), torch.empty_like(v), torch.empty_like(a), torch.empty_like(loc)
    ws = torch.empty(v.numel(), dtype=torch.float32, device=DEV) if dtype else None
    sizes = (N, S, M, D, Lq, L, P)
    ins = (ptr(v), ptr(c["shapes"]), ptr(c["lsi"]), ptr(loc), ptr(a))
    if name == "f32":
        def fwd():
            lib.call("dpft_msda_fwd_f32", *ins, ptr(out), *sizes, stream())

        def bwd():
            gv.zero_()
            lib.call("dpft_msda_bwd_f32", *ins, ptr(go), ptr(gv), ptr(gl), ptr(ga), *sizes, stream())
    else:
        def fwd():
            lib.call("dpft_msda_fwd_typed", *ins, ptr(out), *sizes, dtype, 1, stream())

        def bwd():
            lib.call("dpft_msda_bwd_typed", *ins, ptr(go), ptr(gv), ptr(gl), ptr(ga), ptr(ws), *sizes, dtype, 1, stream())
    return fwd, bwd, {"out": out, "grad_value": gv, "grad_loc": gl, "grad_attn": ga, "keep": (v, a, go, ws)}


def timed(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in ev]


say(f"msda_bench: {torch.cuda.get_device_name(0)}; N {N} M {M} D {D} P {P} levels {SHAPES} S {S}; "
    f"{args.blocks} blocks x {args.reps} timed calls per variant, variants alternating; times in microseconds")
VARIANTS = ("f32", "typed0", "typed1", "typed2")
for Lq in (S, 300):
    c = make_case(Lq)
    var = {n: variant(c, n) for n in VARIANTS}
    for n in VARIANTS:                                   # warm-up: code objects, first launches
        for _ in range(5):
            var[n][0]()
            var[n][1]()
    torch.cuda.synchronize()
    say()
    say(f"Lq = {Lq} ({'encoder' if Lq == S else 'decoder'} form); largest |typed - f32 kernel| on the same inputs (16-bit: inputs rounded first):")
    ref = var["f32"][2]
    for n in VARIANTS[1:]:
        say(f"  {n:7s} " + "  ".join(f"{k} {float((var[n][2][k].float() - ref[k]).abs().max()):.3e} (max|f32| {float(ref[k].abs().max()):.3e})"
                                      for k in ("out", "grad_value", "grad_loc", "grad_attn")))
    us = {(n, d): [] for n in VARIANTS for d in (0, 1)}
    for _ in range(args.blocks):
        for d in (0, 1):
            for n in VARIANTS:
                us[(n, d)] += timed(var[n][d], args.reps)
    floor_us = N * Lq * M * L * P * 4 * D * 4 / ATOMIC_RATE * 1e6
    base = {d: statistics.median(us[("f32", d)]) for d in (0, 1)}
    say(f"  {'variant':8s} {'forward median':>15s} {'min':>9s} {'f32 / it':>9s}   {'backward median':>15s} {'min':>9s} {'f32 / it':>9s} "
        f"{'atomic floor':>13s} {'median / floor':>15s}")
    for n in VARIANTS:
        f, b = us[(n, 0)], us[(n, 1)]
        fm, bm = statistics.median(f), statistics.median(b)
        say(f"  {n:8s} {fm:15.1f} {min(f):9.1f} {base[0] / fm:9.2f}   {bm:15.1f} {min(b):9.1f} {base[1] / bm:9.2f} {floor_us:13.1f} {bm / floor_us:15.2f}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
