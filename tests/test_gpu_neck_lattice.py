"""The FPN neck and its positional embedding (dpft_amd/models/necks/fpn.py, embeddings/sinusoidal.py) against the fp64 oracle over the
lattice of tests/neck_lattice.py.  The CPU half (tests/test_neck_lattice.py) shows that the table reaches what it claims and that
the fp64 oracle follows the float index rule.  Per point of the neck that nothing else in the suite would notice going wrong, the
case that reaches it:

  1  the nearest-upsample index rule: radar-5 (46 -> 14, 44 -> 26 in conv1x1_to16_kernel<6, true>), float-rule-generic (58 -> 30,
     46 -> 28 in fpn_topdown_add_kernel); the gather of fpn_topdown_add_bwd_kernel at all four pairs through the input and
     lateral gradients of the level above
  2  the backward's schedule: cotangents on the top only / level 0 only / all but the middle level, inputs without a gradient at
     every level (params-only) and at level 0, the g_prev chain over five levels (radar-5), weight_transpose_many over the output
     convs alone (params-only)
  3  grad_direct: test_gradients_written_into_the_bucket_arena, every case, all outputs used and the middle one unused
  4  ops.grad_sink: test_input_gradient_written_into_a_registered_sink, every case, bottom and top level
  5  neck(f, pos=..., out_buffers=...): test_values_and_forms, every case
  6  C = 3: camera-3 (K = 16: fused lateral, thin weight gradient with the bias column), k32 (generic); out_channels 32 and 8: k32, k8
  7  TH == H / TW == W: same-size; a 1x1 top map: radar-5; one level: single; channel_last=False: test_channel_first, every case
  8  conv1x1_to16_kernel's second grid-stride step: test_fused_lateral_above_one_grid_stride_step (1 x 520 x 510, C = 3)

The bound is the project's rule for "a different but equally rounded evaluation": distance to the fp64 value <= max(floor, 4 e32),
e32 = the fp32 CPU evaluation of the same oracle against fp64, recomputed here; floors 1e-5 (outputs) and 1e-4 (gradients); held
per tensor in rel-L2 and in the largest element-wise error over max |ref|, e32 in the same norm.  Both distances and their ratio
are printed for every case and tensor group.  Bit equality is asserted where the kernels and their order are the same by
construction: the embedding in the 3x3 conv's epilogue against conv + add_pos, output buffers, a repeated run (no atomics), the
channel-first form (same kernels behind a layout change), gradients that do not depend on which inputs need one, bucket views
and sinks against the tensors autograd would have received.

Measured on an MI355X, worst ratio gpu / e32 over cases and tensors, rel-L2 | max norm: outputs 1.08 (single, level 0) | 1.52
(same-size, level 2); gradients, all forms and partial uses 2.13 (k8 inner_blocks.1 bias, 1.6e-7 against 7.7e-8) | 1.94 (k8
inner_blocks.1 weight); with the fused forms switched off outputs 1.01 | 1.30, gradients 1.48 | 1.58; the fused lateral at 265 200
pixels 1.00 | 1.00 (it rounds as the fp32 oracle does).  The largest distances are 3.9e-7 | 6.5e-7 (outputs) and 3.6e-7 | 5.5e-7
(gradients): every tensor sits more than a decade under its floor, nothing needed more than the bound, and every bit equality
held; nothing in the module or its kernels had to change.  Not asserted, only printed: the raw-input level's output of the
process with the switches off was bit-equal to the fused one as well (the thin lateral kernel sums c ascending, bias last, top
last, as the generic path does)."""
import os
import subprocess
import sys

import pytest
import torch

from tests import neck_driver as D
from tests import neck_lattice as L

pytestmark = pytest.mark.gpu
DEV = D.DEV
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plain():
    """The plain form emb(neck(f)) of every case, all cotangents, every input with a gradient: run once, left unchanged."""
    cache = {}

    def get(c):
        if c.name not in cache:
            cache[c.name] = D.run(c, "plain")
        return cache[c.name]
    return get


@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_values_and_forms(c, plain):
    """Outputs, every parameter gradient and every input gradient (level 0 included) against fp64; then the forms the model
    calls -- the embedding handed to the neck, the same into output buffers -- and a second run, bit-equal to the plain form."""
    base = plain(c)
    assert [tuple(o.shape) for o in base["outs"]] == L.out_shapes(c)
    D.check_run(c, "plain", base)
    D.equal_runs(c, "second run", D.run(c, "plain"), base)
    D.equal_runs(c, "pos", D.run(c, "pos"), base)
    r = D.run(c, "buffers")
    assert [o.data_ptr() for o in r["outs"]] == [b.data_ptr() for b in r["buffers"]]
    D.equal_runs(c, "pos + out_buffers", r, base)
    D.equal_runs(c, "pos + out_buffers, second run", D.run(c, "buffers"), base)


@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_channel_first(c, plain):
    """channel_last=False: NCHW in, NCHW out, the values of the channel-last form; the fused embedding is refused."""
    last = D.run(c, "neck-only")
    D.check_run(c, "neck only", last, neck_only=True)
    D.equal_runs(c, "neck only: gradients", last, plain(c), outputs=False)      # the embedding's backward is the identity
    first = D.run(c, "neck-only", channel_last=False)
    assert [tuple(o.shape) for o in first["outs"]] == [(B, K, H, W) for B, H, W, K in L.out_shapes(c)]
    first["outs"] = [o.movedim(1, -1) for o in first["outs"]]
    D.check_run(c, "channel-first", first, neck_only=True)
    D.equal_runs(c, "channel-first", first, last)
    emb = L.embedding(c)
    feats = {str(i): x.detach() for i, x in enumerate(first["inputs"])}
    nhwc = {k: v.movedim(1, -1) for k, v in feats.items()}
    with pytest.raises(ValueError, match="channel-last"):
        first["neck"](feats, pos=emb.level_tables(nhwc, c.out))


@pytest.mark.parametrize("c", [c for c in L.CASES if L.n_levels(c) > 1], ids=L.case_id)
def test_partial_use(c, plain):
    """Cotangents on part of the outputs, inputs without a gradient: the 3x3 conv of an unused level (and whatever lies below
    every used level) gets exactly zero, everything else is the oracle's; a parameter's gradient does not depend on which
    inputs need one."""
    for cots in L.cot_sets(c):
        full = plain(c) if cots == "all" else D.run(c, "plain", cots)
        if cots != "all":
            D.check_run(c, f"cotangents {cots}", full, cots)
            assert any(not bool(g.any()) for g in full["grads"].values())
        for needs in L.NEEDS[1:]:
            r = D.run(c, "pos" if needs == "params-only" else "plain", cots, needs)
            D.check_run(c, f"cotangents {cots}, inputs {needs}", r, cots, needs)
            for n, g in r["grads"].items():
                if g is not None:
                    assert torch.equal(g, full["grads"][n]), (c.name, cots, needs, n)


class _Spy:
    """Counts what a reducer and autograd are told."""

    def __init__(self, red, params):
        self.calls, self.accumulated = [], 0
        inner = red.mark_ready_many

        def mark_ready_many(ps):
            ps = list(ps)
            self.calls.append([id(p) for p in ps])
            return inner(ps)
        red.mark_ready_many = mark_ready_many
        self.hooks = [p.register_hook(self._hook) for p in params]

    def _hook(self, g):          # (autograd calls a leaf's hook with None where the node returned no gradient for it)
        self.accumulated += g is not None


@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_gradients_written_into_the_bucket_arena(c, plain):
    """grad_direct: a one-process GradBucketReducer over the neck's parameters, announced as overwritten (reset() does not clear
    them), their arena spans filled with NaN.  After forward + backward every bucket view equals the gradient autograd would have
    carried, through the view's logical shape; no NaN is left (written, not added); autograd accumulated nothing; the reducer
    heard mark_ready_many once, with all parameters, each ready once.  Again with the middle level unused: its views are zero."""
    from dpft_amd.training.distributed import GradBucketReducer
    n = L.n_levels(c)
    for cots in ["all"] + (["no-mid"] if n > 2 else ["top"] if n > 1 else []):
        ref = plain(c) if cots == "all" else D.run(c, "plain", cots)
        neck = L.module(c).to(DEV)
        params = list(neck.parameters())
        red = GradBucketReducer(params)
        assert len(red.params) == 4 * n
        red.set_overwritten(neck.overwritten_parameters())
        neck.grad_direct = red
        for step in range(2):           # the second step finds the first one's gradients in the arena, not zeros or NaN
            red.reset()
            if step == 0:
                for p in params:
                    red.grad_buffer(p).fill_(float("nan"))
                assert bool(torch.isnan(red.arena).any())
            spy = _Spy(red, params)
            r = D.run(c, "pos", cots, neck=neck)
            for h in spy.hooks:
                h.remove()
            del red.mark_ready_many
            assert not bool(torch.isnan(red.arena).any()), (c.name, cots, step)
            assert spy.accumulated == 0 and len(spy.calls) == 1 and sorted(spy.calls[0]) == sorted(id(p) for p in params)
            assert red.seen_ids() == {id(p) for p in params}
            assert all(b["ready"] == len(b["params"]) and b["fired"] for b in red.buckets)
            for name, p in neck.named_parameters():
                view = red.grad_buffer(p)
                assert p.grad is view and tuple(view.shape) == tuple(p.shape), name
                if p.dim() == 4:        # physically [K][kh][kw][C] inside the arena
                    assert view.permute(0, 2, 3, 1).is_contiguous() and p.permute(0, 2, 3, 1).is_contiguous(), name
                a, b = red._spans[id(p)]
                assert view.data_ptr() == red.arena[a:b].data_ptr() and b - a == p.numel()
                assert torch.equal(view.cpu(), ref["grads"][name]), (c.name, cots, step, name)
                if name in L.zero_grads(c, L.cot_sets(c)[cots]):
                    assert not bool(view.any()), (c.name, cots, name)
            for i in range(n):
                assert torch.equal(r["grads"][f"x{i}"], ref["grads"][f"x{i}"]), (c.name, cots, i)
            for o, o_ref in zip(r["outs"], ref["outs"]):
                assert torch.equal(o, o_ref)
        red.remove()


@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_input_gradient_written_into_a_registered_sink(c, plain):
    """ops.grad_sink: with a sink registered for an input level, the lateral's data gradient is written in place into the sink
    and the sink is what autograd receives; values as without a sink."""
    from dpft_amd.hip import ops
    base = plain(c)
    for level in sorted({0, L.n_levels(c) - 1}):
        sink = torch.full(L.level_shapes(c)[level], float("nan"), device=DEV)
        seen = []

        def before_backward(neck, inputs, level=level, sink=sink, seen=seen):
            ops.register_grad_sink(inputs[level], sink)
            inputs[level].register_hook(lambda g: seen.append(g.data_ptr()))
            for i, x in enumerate(inputs):
                assert (ops.grad_sink(x) is sink) == (i == level)

        r = D.run(c, "pos", before_backward=before_backward)
        try:
            assert seen == [sink.data_ptr()], (c.name, level)
            assert torch.equal(sink.cpu(), base["grads"][f"x{level}"]), (c.name, level)
            D.equal_runs(c, f"sink at level {level}", r, base)
        finally:
            ops.drop_grad_sink(r["inputs"][level])
        assert ops.grad_sink(r["inputs"][level]) is None


def test_fused_lateral_above_one_grid_stride_step():
    """conv1x1_to16_kernel<3, true> at 265 200 pixels: its grid is capped at 4096 blocks of 64 pixels, so the last 3056 pixels are
    a block's second step.  Against fp64 with the float index rule, into a NaN-filled buffer (a pixel the loop skips stays NaN);
    and a 40 x 57 crop of the same operands against its own reference, which places a failure: both fail = the kernel's
    arithmetic, only the large one = the loop."""
    from dpft_amd.hip import ops
    k, t = L.KERNEL_CASE, L.kernel_case()
    c = L.Case("to16-grid-stride", (k["C"],), ((k["H"], k["W"]),), k["K"], k["B"], 11)
    dev = {n: t[n].to(DEV) for n in ("x", "top", "w", "b")}

    def lateral(x, top):
        B, H, W, C = x.shape
        out = torch.full((B, H, W, k["K"]), float("nan"), device=DEV)
        got = ops.fpn_lateral(ops.conv_problem(B, H, W, C, k["K"], 1, 1, 1, 0), x.contiguous(), dev["w"], dev["b"], top=top.contiguous(), out=out)
        assert got.data_ptr() == out.data_ptr()
        return got

    h, w = k["crop"]
    th, tw = h // 2, (w + 1) // 2
    xc, tc = t["x"][:, :h, :w].contiguous(), t["top"][:, :th, :tw].contiguous()
    rows = []
    D.check(c, "crop", f"lateral {h}x{w}", lateral(xc.to(DEV), tc.to(DEV)), L.lateral_reference(xc, tc, t["w"], t["b"], torch.float64),
            L.lateral_reference(xc, tc, t["w"], t["b"], torch.float32), D.FLOOR_OUT, rows)
    D.summary(c, "fused lateral, crop", rows)
    rows = []
    got = lateral(dev["x"], dev["top"])
    assert got.shape[1] * got.shape[2] > L.TO16_CAP
    tail = got.flatten(0, 2)[L.TO16_CAP:]
    assert bool(torch.isfinite(tail).all()), "pixels of the second grid-stride step were not written"
    D.check(c, "full", "lateral 520x510", got, t["ref64"], t["ref32"], D.FLOOR_OUT, rows)
    D.check(c, "full", "lateral 520x510, second step", tail, t["ref64"].flatten(0, 2)[L.TO16_CAP:], t["ref32"].flatten(0, 2)[L.TO16_CAP:],
            D.FLOOR_OUT, rows)
    D.summary(c, "fused lateral, 265 200 pixels", rows)


def test_fused_forms_switched_off_in_a_child_process(tmp_path, plain):
    """DPFT_FPN_FUSE=0 DPFT_BIAS_FUSE=0 DPFT_WGRAD16_TILED=0 (read once per process): radar-5 and camera-3 through conv +
    fpn_topdown_add + add_pos, the generic 1x1 weight gradient + bias_grad and the streaming conv16 weight gradient meet the same
    bound.  Bit-equal to the fused process: the outputs of every level whose lateral is the generic kernel in both (all but the
    raw-input level 0, whose thin kernel rounds the 1x1 products on its own), and the 3x3 conv + embedding on a given lateral."""
    path = str(tmp_path / "neck_child.pt")
    env = dict(os.environ, DPFT_FPN_FUSE="0", DPFT_BIAS_FUSE="0", DPFT_WGRAD16_TILED="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "neck_child.py"), path], env=env, capture_output=True, text=True,
                       timeout=300)
    print(p.stdout[-6000:])
    assert p.returncode == 0 and "neck child OK" in p.stdout, (p.stdout[-3000:], p.stderr[-3000:])
    saved = torch.load(path)
    for name in L.CHILD:
        c = L.by_name(name)
        base = plain(c)
        assert L.fused_lateral(c, 0) and not any(L.fused_lateral(c, i) for i in range(1, L.n_levels(c)))
        for form in ("plain", "pos"):
            r = saved[(name, form)]
            D.check_run(c, f"switches off, {form}", dict(outs=r["outs"], grads=r["grads"]))
            for i in range(1, L.n_levels(c)):
                assert torch.equal(r["outs"][i], base["outs"][i].cpu()), (name, form, i)
            print(f"{name}: level 0 output of the unfused process bit-equal to the fused one: {torch.equal(r['outs'][0], base['outs'][0].cpu())}")
        assert torch.equal(saved[(name, "probe")], D.probe_output_conv(c)), name
