"""TEST INFRASTRUCTURE -- the lattice of tests/test_plan_lattice.py (CPU) and tests/test_gpu_plan_lattice.py (GPU).

The native ResNet launch plan (dpft_amd/csrc/resnet_plan.hip) strings the conv, BatchNorm and glue kernels together: which
activation buffer and dy slot a block uses (g_cur / dyi = blocks of the later stages & 1), which BatchNorm is still pending as
column sums and who may read the sums, whether a block's bn3 reduction rides in the previous data-gradient kernel (nextb), the
identity branch with and without a downsample, the row count M of every BatchNorm, the stem's pooled size, the eval epilogue
path, the frozen-BatchNorm path, the three act16 storage forms, and when the running statistics are written.  The kernels are
pinned one by one elsewhere; here the plan is, on SHALLOW bodies: one to three bottlenecks per stage are a short, well-conditioned
chain, on which every output, running statistic and parameter gradient can be held to fp32 round-off of the fp64 oracle.

What each case reaches (maps follow floor((n - 1) / 2) + 1 at the stem, the pool and each strided 3x3):

  odd-wide   (2,1,2,1) ms 4, 6 ch, 2x33x70   odd stem 17x35, pool 9x18 (even width), several statistics tiles with a ragged last
                                             one, the adjustment conv and its gradient, nextb folded once in stages 1 and 3,
                                             blocks-in-later-stages 4 / 3 / 1 / 0
  l4-2x1     (1,1,1,1) ms 4, 3 ch, 2x35x27   even stem 18x14, odd pool 9x7, a 2x1 layer4 map: M = 4, the smallest admitted
  b4-1x1     (1,1,1,1) ms 4, 3 ch, 4x17x17   odd stem 9, odd pool 5, a 1x1 layer4 map at batch 4; later blocks 3 / 2 / 1 / 0
  parity     (1,2,1,2) ms 4, 3 ch, 6x17x23   later blocks 5 / 3 / 2 / 0: with the rows above both parities for stages 1..3 (the
                                             last stage of a body always starts at 0); a 1x1 layer4 map with a second block.
                                             Batch 6, not 4: two layer4 blocks normalising over 4 rows put the fp32 oracle at
                                             3e-5 .. 5e-5 (outputs) and 2e-4 .. 6e-4 (gradients) of fp64 at every seed tried
  b1         (2,2)     ms 2, 6 ch, 1x21x40   a batch of one, two stages, even pool 6x10
  l3only     (1,1,2)   ms 3, 3 ch, 2x29x45   three stages
  l1only     (3,)      ms 1, 6 ch, 2x19x26   a stage of three blocks (nextb folded twice, two residual data gradients without a
                                             downsample), the stem in the same backward call as the only stage
  even-2x2   (1,1,1,1) ms 4, 6 ch, 2x64x64   every map even, M a multiple of every tile (2048, 512, 128, 32, 8): the control

The statistics tile of a conv is one row block of its GEMM (dpft_conv2d_stats_tiles: 64 to 256 rows); the elementwise passes
walk rows in blocks of the same order.  The table's row counts run from 4 to 2048: below one tile (4, 6, 8, 12, 15, 16, ...), several
tiles with a ragged last one (1190, 690, 648, 324, 260, ...) and exact multiples (2048, 512, 128), so no case was added for them.

ReLU decisions are kept away from zero (condition()): with random parameters about one (case, seed) in five has a ReLU input
within fp32 round-off of zero somewhere, and that one flipped mask element moves the gradients of a block by 1e-3 to 3e-2 where
the same case without a flip sits at 1e-5.  A seed can be chosen so that the fp32 CPU oracle has no flip, but the GPU rounds
differently and flips as often on its own.  In train mode the ReLU input of channel c is gamma_c zhat + beta_c (+ the identity
for bn3) and zhat does not depend on beta_c: the fp64 forward is walked layer by layer and, at every BatchNorm that feeds a ReLU,
beta_c moves to the middle of the widest gap among the zeros of that channel next to the drawn beta_c.  In eval / frozen mode the
same shift works with the running statistics, so each (case, BatchNorm mode) has its own conditioned state.  The stem max-pool
has no such handle (which of two near-equal entries of a window wins): that is met by the case's seed -- the first of 1, 2, ...
at which the smallest top-2 gap is 12x the deviation or more, so that the asserted 8x does not hang on one machine's fp32 sums.

One fp64 walk of the body (walk) serves the conditioning, the references and the bf16 yardstick: it taps every pre-BatchNorm,
pre-ReLU and pre-pool tensor, and takes an operand quantiser (the conv) and a storage quantiser.  Without hooks it returns exactly
what oracle.dprt_oracle.resnet_body returns (CPU half).  ``python -m tests.plan_lattice`` prints the table and the margins."""
from collections import OrderedDict, namedtuple

import torch
import torch.nn.functional as F

from oracle import dprt_oracle as O

Case = namedtuple("Case", "name depths multi_scale in_ch B H W seed")

CASES = [
    Case("odd-wide", (2, 1, 2, 1), 4, 6, 2, 33, 70, 3),
    Case("l4-2x1", (1, 1, 1, 1), 4, 3, 2, 35, 27, 1),
    Case("b4-1x1", (1, 1, 1, 1), 4, 3, 4, 17, 17, 1),
    Case("parity", (1, 2, 1, 2), 4, 3, 6, 17, 23, 2),
    Case("b1", (2, 2), 2, 6, 1, 21, 40, 1),
    Case("l3only", (1, 1, 2), 3, 3, 2, 29, 45, 1),
    Case("l1only", (3,), 1, 6, 2, 19, 26, 1),
    Case("even-2x2", (1, 1, 1, 1), 4, 6, 2, 64, 64, 1),
]
MODES = ("train", "eval")                         # BatchNorm from the batch statistics | from the running statistics
PARTIAL = ("odd-wide", "l3only", "l1only", "parity")      # cotangents on part of the outputs
BF16 = ("even-2x2", "odd-wide", "l1only")         # bf16 compute with act16 0, 1, 2
PLANES = (64, 128, 256, 512)
EPS, MOMENTUM = 1e-5, 0.1
P = "bb"                                          # key prefix of the oracle's state dict
MARGIN = 8.0                                      # min |ReLU input| / fp32 deviation at that tensor; pool top-2 gap likewise
CAP_OUT, CAP_GRAD = 2e-5, 2e-4                    # the fp32 oracle's rel-L2 error may not exceed these (conditioning of a case)
NEIGHBOURS = 3                                    # zeros looked at on either side of the drawn beta


def by_name(name):
    return next(c for c in CASES if c.name == name)


def case_id(c):
    return c.name


def half(n):
    return (n - 1) // 2 + 1


def geometry(c):
    """(stem map, pool map, [stage maps])."""
    stem = (half(c.H), half(c.W))
    h, w = pool = (half(stem[0]), half(stem[1]))
    stages = []
    for li in range(len(c.depths)):
        if li > 0:
            h, w = half(h), half(w)
        stages.append((h, w))
    return stem, pool, stages


def stage_shapes(c):
    """NHWC shapes of the stage outputs."""
    return [(c.B, h, w, 4 * PLANES[li]) for li, (h, w) in enumerate(geometry(c)[2])]


def bn_layers(c):
    """[(name, channels, rows M, feeds a ReLU)] of every BatchNorm in the plan's table order."""
    stem, pool, stages = geometry(c)
    rows = lambda hw: c.B * hw[0] * hw[1]
    out = [("body.bn1", 64, rows(stem), True)]
    prev = pool
    for li, n in enumerate(c.depths):
        for b in range(n):
            q = f"body.layer{li + 1}.{b}"
            out += [(q + ".bn1", PLANES[li], rows(prev), True), (q + ".bn2", PLANES[li], rows(stages[li]), True),
                    (q + ".bn3", 4 * PLANES[li], rows(stages[li]), True)]
            if b == 0:
                out.append((q + ".downsample.1", 4 * PLANES[li], rows(stages[li]), False))
            prev = stages[li]
    return out


def n_convs(c):
    return (c.in_ch != 3) + 1 + sum(3 * n + 1 for n in c.depths)


def later_blocks(c):
    """Per stage index: the blocks of the later stages (resnet_plan.hip: g_cur = dyi = this & 1 at the start of the stage)."""
    return [sum(c.depths[li + 1:]) for li in range(len(c.depths))]


def cot_sets(c):
    """Which stage outputs get a cotangent: all; on the PARTIAL cases also only the last, and only a middle one."""
    n = len(c.depths)
    sets = OrderedDict(all=tuple(range(n)))
    if c.name in PARTIAL:
        sets["last"] = (n - 1,)
        if n > 1:
            sets["mid"] = (1,)
    return sets


# ------------------------------------------------------------------------------------------------------------------------------
# the one walk of the body
# ------------------------------------------------------------------------------------------------------------------------------
def walk(x, sd, p, depths, train, multi_scale=4, tap=None, conv=None, store=None, before_bn=None):
    """oracle.dprt_oracle.resnet_body with hooks.  tap(kind, name, tensor) sees every "bn_in" (pre-BatchNorm), "relu_in"
    (pre-ReLU) and "pool_in" (pre-pool) tensor; conv(x, w, name, **kw) replaces F.conv2d (the operand quantiser);
    store(tensor, name) is applied to what the plan keeps in HBM between kernels (the storage quantiser);
    before_bn(name, x, identity) runs in front of a BatchNorm that feeds a ReLU and may rewrite its bias in sd."""
    tap = tap or (lambda kind, name, t: None)
    conv = conv or (lambda x, w, name, **kw: F.conv2d(x, w, **kw))
    store = store or (lambda t, name: t)

    def bn(x, name, identity=None, relu=True):
        tap("bn_in", name, x)
        if before_bn is not None and relu:
            before_bn(name, x, identity)
        return O._bn(x, sd, name, train)

    x = conv(x, sd[p + ".conv1.weight"], p + ".conv1", stride=2, padding=3)
    x = bn(x, p + ".bn1")
    tap("relu_in", p + ".bn1", x)
    x = F.relu(x)
    tap("pool_in", p + ".bn1", x)
    x = store(F.max_pool2d(x, kernel_size=3, stride=2, padding=1), p + ".pool")
    out = OrderedDict()
    for li, nblocks in enumerate(depths):
        for b in range(nblocks):
            q = f"{p}.layer{li + 1}.{b}"
            stride = 2 if (li > 0 and b == 0) else 1
            y = store(conv(x, sd[q + ".conv1.weight"], q + ".conv1"), q + ".conv1")
            y = bn(y, q + ".bn1")
            tap("relu_in", q + ".bn1", y)
            y = store(conv(F.relu(y), sd[q + ".conv2.weight"], q + ".conv2", stride=stride, padding=1), q + ".conv2")
            y = bn(y, q + ".bn2")
            tap("relu_in", q + ".bn2", y)
            y = store(conv(F.relu(y), sd[q + ".conv3.weight"], q + ".conv3"), q + ".conv3")
            if (q + ".downsample.0.weight") in sd:
                idn = store(conv(x, sd[q + ".downsample.0.weight"], q + ".downsample.0", stride=stride), q + ".downsample.0")
                idn = bn(idn, q + ".downsample.1", relu=False)
            else:
                idn = x
            y = bn(y, q + ".bn3", identity=idn)
            y = y + idn
            tap("relu_in", q + ".bn3", y)
            x = F.relu(y)
            if b == nblocks - 1 and li < multi_scale:
                out[str(li + 1)] = x
            x = store(x, q + ".out")
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# inputs, parameters, conditioning
# ------------------------------------------------------------------------------------------------------------------------------
def drawn_state(c, seed=None):
    """(fp32 state dict with the oracle's key prefix, fp32 input (B, H, W, C)) as drawn: the module's own initialisation,
    BatchNorm affine parameters and running buffers as test_gpu_model.randomise_bn draws them, input = rand * 255."""
    from dpft_amd.models.backbones.resnet import BackboneBase
    seed = c.seed if seed is None else seed
    g = torch.Generator().manual_seed(seed)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        bb = BackboneBase(c.depths, c.in_ch, c.multi_scale)
    with torch.no_grad():
        for m in bb.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) * 0.5 + 0.75)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) * 0.5 + 0.75)
    x = torch.rand(c.B, c.H, c.W, c.in_ch, generator=g) * 255
    sd = {P + "." + k: v.detach().clone().contiguous() for k, v in bb.state_dict().items()}
    return sd, x


def _body_input(x_nhwc, sd):
    x = x_nhwc.movedim(-1, 1)
    if (P + ".adjustment_layer.weight") in sd:
        x = F.conv2d(x, sd[P + ".adjustment_layer.weight"])
    return x


def _widest_gap_beta(v, beta):
    """v: (C, n) the ReLU input without beta; beta: (C,) as drawn.  The zeros of channel c lie at beta = -v[c, i]: the middle
    of the widest gap among the NEIGHBOURS zeros on either side of the drawn value (beyond the outermost zero: one mean gap)."""
    K = NEIGHBOURS
    t = (-v).sort(dim=1).values.contiguous()
    n = t.shape[1]
    d = ((t[:, -1] - t[:, 0]) / max(n - 1, 1)).clamp_min(1e-3 * (1 + t.abs().amax(1)))
    padded = torch.cat([(t[:, :1] - d[:, None]).expand(-1, K), t, (t[:, -1:] + d[:, None]).expand(-1, K)], dim=1)
    j = torch.searchsorted(t, beta[:, None].contiguous())                # zeros below the drawn beta: t[j - 1] < beta <= t[j]
    idx = j + torch.arange(2 * K)[None, :]                                # padded[j + k] = t[j - K + k]
    win = padded.gather(1, idx)
    gaps = win[:, 1:] - win[:, :-1]
    g = gaps.argmax(dim=1, keepdim=True)
    return (0.5 * (win.gather(1, g) + win.gather(1, g + 1)))[:, 0]


def condition(c, sd32, x, train):
    """The conditioned copy of a drawn state for one BatchNorm mode: an fp64 walk that rewrites the bias of every BatchNorm
    feeding a ReLU (fp32 values)."""
    sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd32.items()}

    def before_bn(name, y, identity):
        if train:
            mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
        else:
            mean, var = sd[name + ".running_mean"], sd[name + ".running_var"]
        zhat = (y - mean[None, :, None, None]) / torch.sqrt(var + EPS)[None, :, None, None]
        v = sd[name + ".weight"][None, :, None, None] * zhat
        if identity is not None:
            v = v + identity
        v = v.movedim(1, 0).reshape(v.shape[1], -1)
        sd[name + ".bias"] = _widest_gap_beta(v, sd[name + ".bias"]).float().double()

    with torch.no_grad():
        walk(_body_input(x.double(), sd), sd, P + ".body", c.depths, train, c.multi_scale, before_bn=before_bn)
    return {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------------------------------------
# evaluation: outputs, taps, gradients
# ------------------------------------------------------------------------------------------------------------------------------
def _round_bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


class _QuantConv(torch.autograd.Function):
    """conv2d with both operands rounded to bf16 (round to nearest even) in the forward and in the two backward products."""

    @staticmethod
    def forward(ctx, x, w, stride, padding):
        ctx.save_for_backward(x, w)
        ctx.geom = (stride, padding)
        return F.conv2d(_round_bf16(x), _round_bf16(w), stride=stride, padding=padding)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        stride, padding = ctx.geom
        g = _round_bf16(g)
        dx = torch.nn.grad.conv2d_input(x.shape, _round_bf16(w), g, stride=stride, padding=padding)
        dw = torch.nn.grad.conv2d_weight(_round_bf16(x), w.shape, g, stride=stride, padding=padding)
        return dx, dw, None, None


class _Stored(torch.autograd.Function):
    """A tensor (and its gradient) the plan keeps as bf16 in HBM."""

    @staticmethod
    def forward(ctx, t):
        return _round_bf16(t)

    @staticmethod
    def backward(ctx, g):
        return _round_bf16(g)


def quant_conv(x, w, name, stride=1, padding=0):
    """The operand quantiser: every body conv with C % 64 == 0 (the stem's C = 3 stays fp32)."""
    if x.shape[1] % 64 != 0:
        return F.conv2d(x, w, stride=stride, padding=padding)
    return _QuantConv.apply(x, w, stride, padding)


def quant_store(t, name):
    return _Stored.apply(t)


def evaluate(c, sd32, x, train, dtype, conv=None, store=None):
    """One evaluation of the oracle walk in `dtype` -> dict(outs (NHWC), taps {kind: {name: tensor}}, grads {cot set: {key:
    tensor}}).  Cotangents: cotangents(c)."""
    leaf = lambda k, v: v.is_floating_point() and "running" not in k
    sd = {k: (v.to(dtype).clone().requires_grad_(True) if leaf(k, v) else (v.to(dtype) if v.is_floating_point() else v))
          for k, v in sd32.items()}
    taps = dict(bn_in=OrderedDict(), relu_in=OrderedDict(), pool_in=OrderedDict())

    def tap(kind, name, t):
        taps[kind][name[len(P) + 1:]] = t.detach()

    feats = walk(_body_input(x.to(dtype), sd), sd, P + ".body", c.depths, train, c.multi_scale, tap=tap, conv=conv, store=store)
    outs = OrderedDict((k, v.movedim(1, -1)) for k, v in feats.items())
    cots = cotangents(c)
    leaves = [k for k, v in sd.items() if leaf(k, v)]
    grads = OrderedDict()
    for name, stages in cot_sets(c).items():
        loss = sum((outs[str(li + 1)] * cots[li].to(dtype)).sum() for li in stages)
        gs = torch.autograd.grad(loss, [sd[k] for k in leaves], retain_graph=True, allow_unused=True)
        grads[name] = {k[len(P) + 1:]: (torch.zeros_like(sd[k]) if g is None else g).detach() for k, g in zip(leaves, gs)}
    return dict(outs=OrderedDict((k, v.detach()) for k, v in outs.items()), taps=taps, grads=grads)


def cotangents(c):
    """fp32 random cotangents of the stage outputs (NHWC), one draw per case."""
    g = torch.Generator().manual_seed(1000 + c.seed)
    return [torch.randn(s, generator=g) for s in stage_shapes(c)]


def running_stats(c, sd32, bn_in, steps, dtype=torch.float64):
    """{name: (running_mean, running_var)} after `steps` train forwards of the same input: (1 - m) r + m stat with the
    unbiased variance, from the tapped pre-BatchNorm tensors."""
    out = OrderedDict()
    for name, y in bn_in.items():
        y = y.to(dtype)
        mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=True)
        rm, rv = sd32[f"{P}.{name}.running_mean"].to(dtype), sd32[f"{P}.{name}.running_var"].to(dtype)
        for _ in range(steps):
            rm, rv = (1 - MOMENTUM) * rm + MOMENTUM * mean, (1 - MOMENTUM) * rv + MOMENTUM * var
        out[name] = (rm, rv)
    return out


def rel_l2(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).norm() / (ref.norm() + 1e-30))


def pool_margin(pool64, pool32):
    """(smallest top-2 gap over the stem max-pool windows with a positive maximum, fp32 deviation of the pooled tensor)."""
    win = F.unfold(F.pad(pool64, (1, 1, 1, 1), value=float("-inf")).flatten(0, 1)[:, None], kernel_size=3, stride=2)
    top = win.topk(2, dim=1).values
    gap = (top[:, 0] - top[:, 1])[top[:, 0] > 0]
    return float(gap.min()), float((pool32.double() - pool64).abs().max())


def relu_margins(t64, t32):
    """[(name, min |x| in fp64, max |fp32 - fp64|, sign patterns equal)] over the pre-ReLU tensors."""
    return [(name, float(t.abs().min()), float((t32[name].double() - t).abs().max()), bool(torch.equal(t > 0, t32[name] > 0)))
            for name, t in t64.items()]


_CACHE = {}


def cached(c, mode):
    """(conditioned fp32 state, fp32 input, fp64 evaluation, fp32 evaluation) of a case in a BatchNorm mode; computed once
    and left unchanged."""
    key = (c.name, mode)
    if key not in _CACHE:
        train = mode == "train"
        sd, x = drawn_state(c)
        sd = condition(c, sd, x, train)
        _CACHE[key] = (sd, x, evaluate(c, sd, x, train, torch.float64), evaluate(c, sd, x, train, torch.float32))
    return _CACHE[key]


_CACHE16 = {}


def cached_bf16(c, act16):
    """The yardstick of the bf16 modes: the fp64 walk (train mode) with the operand quantiser on and, for act16 >= 1, the
    stored tensors rounded as well (one emulation for act16 1 and 2: the tensors act16 = 2 materialises are conv operands)."""
    key = (c.name, min(act16, 1))
    if key not in _CACHE16:
        sd, x = cached(c, "train")[:2]
        _CACHE16[key] = evaluate(c, sd, x, True, torch.float64, conv=quant_conv, store=quant_store if act16 else None)
    return _CACHE16[key]


def module(c, mode):
    """A fresh BackboneBase holding the conditioned state (CPU)."""
    from dpft_amd.models.backbones.resnet import BackboneBase
    bb = BackboneBase(c.depths, c.in_ch, c.multi_scale)
    bb.load_state_dict({k[len(P) + 1:]: v for k, v in cached(c, mode)[0].items()})
    return bb


def stage_groups(c, names):
    """{stage index: parameter names}; the stem and the adjustment conv count with stage 0."""
    groups = {li: [] for li in range(len(c.depths))}
    for n in names:
        groups[int(n.split(".")[1][5:]) - 1 if n.startswith("body.layer") else 0].append(n)
    return groups


def report(c, mode):
    sd, x, e64, e32 = cached(c, mode)
    rows = relu_margins(e64["taps"]["relu_in"], e32["taps"]["relu_in"])
    name, lo, dev, _ = min(rows, key=lambda r: r[1] / max(r[2], 1e-300))
    gap, pdev = pool_margin(e64["taps"]["pool_in"]["body.bn1"], e32["taps"]["pool_in"]["body.bn1"])
    e_out = max(rel_l2(e32["outs"][k], e64["outs"][k]) for k in e64["outs"])
    e_grad = max(rel_l2(e32["grads"][s][k], g) for s in e64["grads"] for k, g in e64["grads"][s].items() if float(g.norm()) > 0)
    return (f"{c.name:9s} {mode:5s} seed {c.seed:2d}  min|relu in| {min(r[1] for r in rows):.1e}  max fp32 dev {max(r[2] for r in rows):.1e}"
            f"  tightest {lo / max(dev, 1e-300):7.1f}x at {name}  flips {sum(not r[3] for r in rows)}  pool gap {gap:.1e} / dev {pdev:.1e}"
            f" = {gap / max(pdev, 1e-300):6.1f}x  e32 out {e_out:.1e} grad {e_grad:.1e}")


if __name__ == "__main__":
    for c in CASES:
        stem, pool, stages = geometry(c)
        print(f"{c.name:9s} depths {c.depths} ms {c.multi_scale} in {c.in_ch} {c.B}x{c.H}x{c.W}: stem {stem} pool {pool} stages {stages}"
              f"  M {sorted({m for _, _, m, _ in bn_layers(c)})}  later blocks {later_blocks(c)}")
    for c in CASES:
        for mode in MODES:
            print(report(c, mode))
