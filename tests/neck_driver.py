"""TEST INFRASTRUCTURE -- runs a case of tests/neck_lattice.py through the FPN module on the GPU.  Shared by
tests/test_gpu_neck_lattice.py and its child process tools/neck_child.py (the fused forms switched off: the library reads the
switches once per process)."""
from collections import OrderedDict

import torch

from tests import neck_lattice as L

DEV = "cuda"
FLOOR_OUT, FLOOR_GRAD = 1e-5, 1e-4
FORMS = ("plain", "pos", "buffers", "neck-only")


def run(c, form="plain", cots="all", needs="all", neck=None, channel_last=True, before_backward=None):
    """One forward + backward of a case.  form: "plain" emb(neck(f)) | "pos" neck(f, pos=tables) | "buffers" the same into
    out_buffers | "neck-only" neck(f), no embedding.  cots: a key of L.cot_sets(c); needs: which inputs require a gradient
    (L.NEEDS).  before_backward(neck, inputs): called between the two.  -> dict(outs [device tensors], grads {name: CPU tensor
    or None}, inputs, neck, buffers)."""
    sd, xs, cs, _, _ = L.cached(c)
    if neck is None:
        neck = L.module(c, channel_last).to(DEV)
    emb = L.embedding(c)
    flags = L.x_needs(c, needs)
    inputs = [(x if channel_last else x.movedim(-1, 1).contiguous()).to(DEV).requires_grad_(f) for x, f in zip(xs, flags)]
    feats = OrderedDict((str(i), x) for i, x in enumerate(inputs))
    bufs = None
    if form == "plain":
        outs = emb(neck(feats))
    elif form == "neck-only":
        outs = neck(feats)
    else:
        pos = emb.level_tables(feats, neck.out_channels)
        assert pos is not None and len(pos) == L.n_levels(c)
        if form == "buffers":
            bufs = [torch.full(s, float("nan"), device=DEV) for s in L.out_shapes(c)]
        outs = neck(feats, pos=pos, out_buffers=bufs)
    assert list(outs.keys()) == list(feats.keys())
    outs = list(outs.values())
    if before_backward is not None:
        before_backward(neck, inputs)
    if neck.grad_direct is None:          # (with a reducer attached param.grad are its bucket views)
        neck.zero_grad(set_to_none=True)
    cot = [(t if channel_last else t.movedim(-1, 1)).to(DEV) for t in cs]
    sum((outs[i] * cot[i]).sum() for i in L.cot_sets(c)[cots]).backward()
    torch.cuda.synchronize()
    grads = OrderedDict((n, None if p.grad is None else p.grad.detach().cpu().clone()) for n, p in neck.named_parameters())
    for i, x in enumerate(inputs):
        g = x.grad
        grads[f"x{i}"] = None if g is None else (g if channel_last else g.movedim(1, -1)).detach().cpu().clone()
    return dict(outs=[o.detach() for o in outs], grads=grads, inputs=inputs, neck=neck, buffers=bufs)


def check(c, what, name, got, ref64, ref32, floor, rows):
    """The project's rule in rel-L2 and in the largest element-wise error over max |ref|: gpu <= max(floor, 4 e32)."""
    assert tuple(got.shape) == tuple(ref64.shape), (c.name, what, name, tuple(got.shape))
    assert bool(torch.isfinite(got).all()), (c.name, what, name, "NaN / Inf")
    for norm, fn in (("l2", L.rel_l2), ("max", L.rel_max)):
        e, e32 = fn(got, ref64), fn(ref32, ref64)
        rows.append((e / max(e32, 1e-30), e, e32, f"{name} [{norm}]"))
        assert e <= max(floor, 4 * e32), (c.name, what, name, norm, e, e32)


def summary(c, what, rows):
    for norm in ("l2", "max"):
        sel = [r for r in rows if r[3].endswith(f"[{norm}]")]
        ratio, e, e32, name = max(sel)
        print(f"{c.name:19s} {what:34s} {len(sel):3d} tensors  {norm:3s} worst gpu/e32 {ratio:5.2f} (gpu {e:.2e} e32 {e32:.2e} {name})"
              f"  largest gpu {max(r[1] for r in sel):.2e}")


def check_run(c, what, r, cots="all", needs="all", neck_only=False):
    """Outputs and every gradient of a run against fp64; exact zeros where the table says so."""
    _, _, _, e64, e32 = L.cached(c)
    key = "neck" if neck_only else "outs"
    rows = []
    for i, o in enumerate(r["outs"]):
        check(c, what, f"out {i}", o, e64[key][i], e32[key][i], FLOOR_OUT, rows)
    summary(c, what + " outputs", rows)
    rows = []
    g64, g32 = e64["grads"][cots], e32["grads"][cots]
    zero = L.zero_grads(c, L.cot_sets(c)[cots])
    flags = L.x_needs(c, needs)
    for name, g in r["grads"].items():
        if name.startswith("x") and not flags[int(name[1:])]:
            assert g is None, (c.name, what, name)
            continue
        assert g is not None, (c.name, what, name)
        if name in zero:
            assert not bool(g.any()) and tuple(g.shape) == tuple(g64[name].shape), (c.name, what, name, "not exactly zero")
        else:
            check(c, what, name, g, g64[name], g32[name], FLOOR_GRAD, rows)
    summary(c, what + " gradients", rows)


def equal_runs(c, what, a, b, outputs=True):
    """Bit equality of two runs' outputs and gradients."""
    if outputs:
        for i, (x, y) in enumerate(zip(a["outs"], b["outs"])):
            assert torch.equal(x, y), (c.name, what, f"out {i}", float((x - y).abs().max()))
    assert list(a["grads"]) == list(b["grads"])
    for n in a["grads"]:
        x, y = a["grads"][n], b["grads"][n]
        assert (x is None) == (y is None), (c.name, what, n)
        if x is not None:
            assert torch.equal(x, y), (c.name, what, n, float((x - y).abs().max()))


def probe_output_conv(c):
    """The 3x3 output conv of level 0 with the embedding on a seeded lateral: the tensor a process with the epilogue switched off
    has to reproduce bit for bit (same conv kernel, the same two adds in the same order)."""
    from dpft_amd.hip import ops
    from dpft_amd.models.backbones.resnet import khwc
    neck, emb = L.module(c).to(DEV), L.embedding(c)
    B, H, W, K = L.out_shapes(c)[0]
    lat = torch.randn(B, H, W, K, generator=torch.Generator().manual_seed(100 + c.seed)).to(DEV)
    conv = neck.fpn.layer_blocks[0][0]
    pos = emb.embedding_layers["embedding0"].tables(H, W, lat.device)
    return ops.fpn_output(ops.conv_problem(B, H, W, K, K, 3, 3, 1, 1), lat, khwc(conv.weight), conv.bias, pos=pos).cpu()


def run_child(path):
    """tools/neck_child.py: the CHILD cases with whatever switches the environment sets; distances printed, tensors saved."""
    import os
    print("switches:", {k: os.environ.get(k) for k in ("DPFT_FPN_FUSE", "DPFT_BIAS_FUSE", "DPFT_WGRAD16_TILED")})
    saved = {}
    for name in L.CHILD:
        c = L.by_name(name)
        for form in ("plain", "pos"):
            r = run(c, form)
            check_run(c, f"child {form}", r)
            saved[(name, form)] = dict(outs=[o.cpu() for o in r["outs"]], grads=r["grads"])
        saved[(name, "probe")] = probe_output_conv(c)
    torch.save(saved, path)
    print("neck child OK")
