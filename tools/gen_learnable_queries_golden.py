"""Generate tests/golden/learnable_queries.npz by running the REFERENCE's own LearnableQueries -> IMPFusion.

    python tools/gen_learnable_queries_golden.py

Like oracle/gen_golden.py it imports the reference's Python through ``oracle.ref_import.install()`` and therefore runs only
where a reference checkout exists.  The fixture is data only:
  queries      the seeded initial parameter (torch.manual_seed(7), the kradar config's resolution / minimum / maximum,
               q_init 'uniform_', transformation spher2cart)       src/dprt/models/queries/learnable.py:95-101
  center       LearnableQueries.forward for B = 2                    src/dprt/models/queries/learnable.py:103-128
  grad_A       queries.grad through the reference's IMPFusion (dropout 0, train mode, the weights and inputs of
               tests/golden/fuser_small.npz) under the cotangents cot/* of tests/golden/fuser_grads.npz
  grad_B       the same with cot/center = 0: the centre gradient then reaches the queries only through the reference points
  loss_A/B     the two scalar losses
"""
from __future__ import annotations

import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
VIEWS = ("camera_mono", "radar_bev", "radar_front")


def main():
    ref_import.install()
    from dprt.models.fusers import build_fuser
    from dprt.models.heads import build_head
    from dprt.models.queries import build_querent

    cfg = json.load(open(os.path.join(ref_import.REFERENCE_SRC, "..", "config", "kradar.json")))
    comp, m = cfg["computing"], cfg["model"]
    small = np.load(os.path.join(GOLDEN, "fuser_small.npz"))
    grads = np.load(os.path.join(GOLDEN, "fuser_grads.npz"))
    T = lambda a: torch.from_numpy(np.asarray(a))      # noqa: E731

    qcfg = {k: m["querent"][k] for k in ("resolution", "minimum", "maximum", "transformation")}
    torch.manual_seed(7)
    querent = build_querent("learnable_querent", dict(comp | qcfg | {"q_init": "uniform_"}))
    B = 2
    out = {"queries": querent.queries.detach().clone()}
    out["center"] = querent({"x": torch.zeros(B, 3)})["center"].detach().clone()

    fcfg = dict(comp | m["fuser"])
    fcfg["dropout"] = 0.0
    fuser = build_fuser(m["fuser"]["name"], fcfg, head=build_head(m["head"]["name"], dict(comp | m["head"])))
    fuser.load_state_dict({k[3:]: T(v) for k, v in small.items() if k.startswith("sd/")})
    fuser.train()
    views = [OrderedDict((str(l), T(small[f"view/{n}/{l}"])) for l in range(5)) for n in VIEWS]
    proj = [(T(small[f"t{v}"]), T(small[f"p{v}"])) for v in range(3)]
    shp = [T(small[f"shape{v}"]) for v in range(3)]
    for tag in ("A", "B"):
        querent.zero_grad(set_to_none=True)
        fuser.zero_grad(set_to_none=True)
        res = fuser(batch=views, shape=shp, projection=proj, out=querent({"x": torch.zeros(B, 3)}))
        cot = {k: T(grads[f"cot/{k}"]) for k in res}
        if tag == "B":
            cot["center"] = torch.zeros_like(cot["center"])
        loss = sum((res[k] * cot[k]).sum() for k in res)
        loss.backward()
        out[f"grad_{tag}"] = querent.queries.grad.detach().clone()
        out[f"loss_{tag}"] = loss.detach().clone()
    np.savez_compressed(os.path.join(GOLDEN, "learnable_queries.npz"), **{k: v.numpy() for k, v in out.items()})
    for k, v in out.items():
        print(k, tuple(v.shape), float(v.double().norm()))


if __name__ == "__main__":
    main()
