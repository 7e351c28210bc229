"""The RCCL exchange path on ONE GPU: a one-rank RCCL communicator (backend "nccl") with every gradient bucket forced
through dist.all_reduce(async_op=True) on RCCL's stream -- stream joins per bucket, ncclAvg, the bf16 wire staging, the
all-ranks step decision, decoder hipGraphs captured next to the RCCL watchdog -- against the plain single-process step on
the same weights and data (a reduction over one rank is the identity).
    python tools/rccl1_forced.py            (env GRAPHS=0/1, WIRE=fp32/bf16, QUERENT=learnable: learned query points)"""
import copy, os, socket, sys, torch
import torch.distributed as dist
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
from dpft_amd.configs import load_config
from dpft_amd.models import build
from dpft_amd.synthetic import make_batch, make_labels
from dpft_amd.training.trainer import DataParallelTrainer

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
with socket.socket() as sk:
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
dist.init_process_group(backend="nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
cfg = load_config("kradar")
cfg["model"]["fuser"]["dropout"] = 0.0
learned = os.environ.get("QUERENT", "static") == "learnable"
if learned:      # LearnableQueries on the static querent's grid: its gradient comes out of the decoder's backward like a pyramid's
    q = cfg["model"]["querent"]
    cfg["model"]["querent"] = {"name": "learnable_querent", "q_init": "uniform_",
                               **{k: q[k] for k in ("resolution", "minimum", "maximum", "transformation")}}
wire = os.environ.get("WIRE", "fp32")
shapes = {"camera_mono": (128, 224, 3), "radar_bev": (128, 43, 6), "radar_front": (37, 107, 6)}
data = make_batch(cfg["model"]["inputs"], 2, seed=7, shapes=shapes, device=dev)
labels = make_labels(2, seed=3, device=dev)

torch.manual_seed(5)
base = build("dprt", cfg)
runs = {}
for name, forced in (("plain", False), ("forced", True)):
    tr = DataParallelTrainer(copy.deepcopy(base), cfg, dev, force_collectives=forced, comm_dtype=wire if forced else None)
    assert tr.collective == forced and tr.reducer.collective == forced
    if os.environ.get("GRAPHS", "1") == "1":
        tr.enable_graphs(data)
    losses, g0 = [], None
    for step in range(3):
        loss, _ = tr.train_step(data, labels)
        losses.append(float(loss))
        if step == 0:      # same weights, same data: the exchanged gradients may differ by the decoder's atomics order only
            torch.cuda.synchronize()
            g0 = torch.cat([b["flat"] for b in tr.reducer.buckets]).clone()
            gq = tr.reducer.grad_buffer(tr.model.querent.queries).clone() if learned else None
    torch.cuda.synchronize()
    if forced:
        assert all(b["fired"] for b in tr.reducer.buckets)
        assert tr.reducer.exposed_ms() >= 0.0
    runs[name] = (losses, [p.detach().clone() for p in tr.model.parameters()], g0)
    if learned:
        runs[name] += (gq, tr.model.querent.queries.detach().clone())
lp, pp, gp = runs["plain"][:3]
lf, pf, gf = runs["forced"][:3]
assert abs(lp[0] - lf[0]) <= 1e-5 * max(1.0, abs(lp[0])), (lp, lf)      # first step: identical weights and data
for a, b in zip(lp, lf):                  # later steps: AdamW's sign-like first updates amplify rounding-level differences
    assert abs(a - b) <= 2e-2 * max(1.0, abs(a)), (lp, lf)
gerr = float((gp.double() - gf.double()).norm() / gp.double().norm())
assert gerr < (1e-2 if wire == "bf16" else 1e-4), gerr       # bf16 wire: one RNE rounding of every gradient (2^-9)
num = sum(float((a.double() - b.double()).pow(2).sum()) for a, b in zip(pp, pf)) ** 0.5
den = sum(float(a.double().pow(2).sum()) for a in pp) ** 0.5
assert num / den < 5e-3, num / den        # three AdamW steps of lr 1e-4 move a parameter by <= 3e-4
print(f"rccl1 forced-collectives OK: wire {wire} losses {lf} param rel diff {num / den:.2e} grad rel diff {gerr:.2e}")
if learned:      # the parameter's gradient was in its bucket when the bucket was exchanged, and the fused AdamW moved it
    (gqp, qp), (gqf, qf) = runs["plain"][3:], runs["forced"][3:]
    qerr = float((gqp.double() - gqf.double()).norm() / gqp.double().norm())
    assert float(gqp.norm()) > 0 and qerr < 5e-4, (float(gqp.norm()), qerr)
    assert not torch.equal(qf, base.querent.queries.detach().to(dev)) and float((qf - qp).abs().max()) < 1e-3
    print(f"learned querent OK: |dqueries| {float(gqp.norm()):.3e} forced vs plain {qerr:.2e}")
dist.barrier()
dist.destroy_process_group()
