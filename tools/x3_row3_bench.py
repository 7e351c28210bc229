"""The split 3x3 GEMMs per launch, each kernel alone: event-timed medians with DPFT_X3_ROW3 (row-shared A stage, conv_x3r.hip)
off and on, alternating twice in one process -- the second column of a pair is the repeat, min / max span all repeats of a form.
Also says whether the two forms' results are bit-equal (they are not: the accumulation order differs) and how far apart.
Run from the repository root:  python tools/x3_row3_bench.py   (numbers: profiles/x3_row3.txt)"""
import os, sys, statistics, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpft_amd.hip import ops
DEV = "cuda"
SHAPES = [(4, 64, 114, 128, 128), (4, 32, 57, 256, 256), (4, 128, 228, 64, 64), (4, 16, 29, 512, 512)]
REP, N = 7, 40

def timed(fn):
    for _ in range(10): fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REP):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(N): fn()
        e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / N)
    return out

for (B, H, W, Cc, K) in SHAPES:
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, H, W, Cc, generator=g).to(DEV); w = (torch.randn(K, 3, 3, Cc, generator=g) / (9 * Cc) ** 0.5).to(DEV)
    dy = torch.randn(B, H, W, K, generator=g).to(DEV); wt = ops.weight_transpose(w)
    bn = torch.stack((torch.randn(Cc, generator=g) * 0.5, torch.rand(Cc, generator=g) + 0.5, torch.rand(Cc, generator=g) * 0.3, torch.ones(Cc))).to(DEV)
    bn_y = torch.randn(B, H, W, Cc, generator=g).to(DEV)
    blk = torch.stack((torch.zeros(Cc), torch.ones(Cc), torch.zeros(Cc), torch.ones(Cc))).to(DEV)
    sums = torch.zeros(2, Cc, device=DEV)
    res = {}
    outs = {}
    for rnd in range(2):
        for sw in ("0", "1"):
            os.environ["DPFT_X3_ROW3"] = sw
            ops._conv_cache.clear()
            cv = ops.conv_problem(B, H, W, Cc, K, 3, 3, 1, 1)
            y = torch.empty(B, H, W, K, device=DEV); dx = torch.empty(B, H, W, Cc, device=DEV)
            forms = {
                "fwd": lambda: ops.conv_fwd(cv, x, w, out=y),
                "fwd+PRO2+stats": lambda: ops.conv_fwd(cv, x, w, pro=(bn, True), want_stats=True, out=y),
                "dgrad": lambda: ops.conv_dgrad(cv, dy, wt, out=dx),
                "dgrad+bnreduce": lambda: ops.conv_dgrad_bn_reduce(cv, dy, wt, bn_y, blk, sums, out=dx),
            }
            for name, fn in forms.items():
                t = timed(fn)
                res.setdefault((name, sw), []).append(t)
                o = (y if name.startswith("fwd") else dx).clone()
                if rnd == 0: outs[(name, sw)] = o
    for name in ("fwd", "fwd+PRO2+stats", "dgrad", "dgrad+bnreduce"):
        line = "%dx%dx%d %d->%d %-16s" % (B, H, W, Cc, K, name)
        for sw in ("0", "1"):
            meds = [statistics.median(t) for t in res[(name, sw)]]
            allv = [v for t in res[(name, sw)] for v in t]
            line += "  row3=%s med %.2f / %.2f us (min %.2f max %.2f)" % (sw, meds[0], meds[1], min(allv), max(allv))
        a, b = outs[(name, "0")], outs[(name, "1")]
        line += "  bit-equal=%s maxdiff=%.2e" % (bool(torch.equal(a, b)), float((a - b).abs().max()))
        print(line, flush=True)
