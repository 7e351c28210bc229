"""TEST INFRASTRUCTURE -- the lattice of tests/test_neck_lattice.py (CPU) and tests/test_gpu_neck_lattice.py (GPU).

The FPN neck (dpft_amd/models/necks/fpn.py) is one autograd node with a hand-scheduled backward over the conv and top-down
kernels: the top-down add rides in the epilogue of the raw-input lateral (conv1x1_to16_kernel<C, TOP>, C = 3 | 6, K = 16), the
positional embedding in the epilogue of the 3x3 output conv (conv16, K = 16); every other shape goes through the generic conv
kernels followed by fpn_topdown_add_kernel / add_pos_kernel.  The backward walks the levels bottom-up with one running gradient
(g_prev), adds the upsample's backward in place into the tensor the 3x3 data gradient just returned, and hands the weight and bias
gradients to autograd or straight into a gradient-bucket arena.  Here the module is held, off the model's shapes, to fp32
round-off of the fp64 oracle (oracle.dprt_oracle.fpn + sinusoidal_embedding, autograd for the gradients).

What each case reaches:

  radar-5             6, 256, 512, 1024, 2048 -> 16   (46,44) (14,26) (5,6) (3,3) (1,1)   B 2
        the float-rule pairs 46 -> 14 (rows) and 44 -> 26 (columns) on the fused C = 6 lateral, a five-level g_prev chain, a 1x1 top
        map (a 3x3 conv on one pixel; every destination of level 3 reads the one source)
  camera-3            3, 64, 128 -> 16                (40,57) (20,29) (10,15)             B 2
        the fused C = 3 lateral, the thin 1x1 weight gradient with the bias as a virtual input channel, conv16 tiles (8 x 32)
        ragged in the width (57 = 32 + 25, five full tile rows: 40 = 5 * 8) and in the height (level 1: 20 = 2 * 8 + 4)
  float-rule-generic  64, 128 -> 16                   (58,46) (30,28)                     B 3
        the float-rule pairs 58 -> 30 and 46 -> 28 through fpn_topdown_add_kernel and the gather of its backward
  same-size           6, 32, 32 -> 16                 (9,12) (9,12) (9,6)                 B 2
        TH == H and TW == W (the fused lateral), then TH == H with TW != W (the generic one)
  single              64 -> 16                        (7,9)                               B 1
        a one-level pyramid: no top-down path, no g_prev
  k32                 3, 64 -> 32                     (16,20) (8,10)                      B 2
        no thin path matches: conv + fpn_topdown_add + add_pos, generic weight gradients + bias_grad
  k8                  6, 32 -> 8                      (11,13) (6,7)                       B 2
        K < 16, num_feats 8

The nearest-upsample index rule is torch's legacy one in fp32, src = min(floorf((float)dst * ((float)in / (float)out)), in - 1)
(float_src); at the pairs above it differs from the exact dst * in // out (exact_src) in one destination each.  The backward's
gather looks for the destinations of a source pixel in a conservative window (candidate_window) and filters by the forward rule;
the CPU half checks that the window contains every destination for all 1 <= in < out < 700.

``python -m tests.neck_lattice`` prints the table, the float-rule destinations and the fp32 yardsticks."""
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from oracle import dprt_oracle as O

Case = namedtuple("Case", "name in_ch sizes out B seed")

CASES = [
    Case("radar-5", (6, 256, 512, 1024, 2048), ((46, 44), (14, 26), (5, 6), (3, 3), (1, 1)), 16, 2, 1),
    Case("camera-3", (3, 64, 128), ((40, 57), (20, 29), (10, 15)), 16, 2, 2),
    Case("float-rule-generic", (64, 128), ((58, 46), (30, 28)), 16, 3, 3),
    Case("same-size", (6, 32, 32), ((9, 12), (9, 12), (9, 6)), 16, 2, 4),
    Case("single", (64,), ((7, 9),), 16, 1, 5),
    Case("k32", (3, 64), ((16, 20), (8, 10)), 32, 2, 6),
    Case("k8", (6, 32), ((11, 13), (6, 7)), 8, 2, 7),
]
FLOAT_RULE = ("radar-5", "float-rule-generic")    # cases with a size pair at which the float rule is not the exact one
CHILD = ("radar-5", "camera-3")                   # run again in a child process with the fused forms switched off
P = "neck"                                        # key prefix of the oracle's state dict
T16H, T16W = 8, 32                                # conv16 kernels: output tile of a workgroup (csrc/conv_plan.h)
TO16_CAP = 256 * 16 * 64                          # conv1x1_to16_kernel: pixels in one step of its grid-stride loop (kNumCU * 16 blocks of 64)
KERNEL_CASE = dict(B=1, H=520, W=510, C=3, K=16, TH=260, TW=255, crop=(40, 57))      # the fused lateral above that cap


def by_name(name):
    return next(c for c in CASES if c.name == name)


def case_id(c):
    return c.name


def n_levels(c):
    return len(c.in_ch)


def level_shapes(c):
    """NHWC shapes of the pyramid's inputs."""
    return [(c.B, h, w, ch) for (h, w), ch in zip(c.sizes, c.in_ch)]


def out_shapes(c):
    return [(c.B, h, w, c.out) for h, w in c.sizes]


def param_names(c):
    return [f"fpn.{blk}.{i}.0.{t}" for blk in ("inner_blocks", "layer_blocks") for i in range(n_levels(c)) for t in ("weight", "bias")]


# ------------------------------------------------------------------------------------------------------------------------------
# the nearest-upsample index rule
# ------------------------------------------------------------------------------------------------------------------------------
def float_src(n_out, n_in):
    """Source index of every destination 0 .. n_out - 1 under the kernels' rule (fp32 scale, fp32 product, floor, clamp)."""
    scale = np.float32(n_in) / np.float32(n_out)
    prod = np.arange(n_out, dtype=np.float32) * scale
    assert prod.dtype == np.float32
    return np.minimum(np.floor(prod).astype(np.int64), n_in - 1)


def exact_src(n_out, n_in):
    return np.arange(n_out, dtype=np.int64) * n_in // n_out


def rule_differs(n_out, n_in):
    """Destinations whose float source is not the exact one."""
    return np.nonzero(float_src(n_out, n_in) != exact_src(n_out, n_in))[0].tolist()


def candidate_window(n_out, n_in):
    """(lo, hi) per source index 0 .. n_in - 1: the destination range fpn_topdown_add_bwd_kernel searches, in its fp32 arithmetic."""
    scale = np.float32(n_in) / np.float32(n_out)
    s = np.arange(n_in, dtype=np.float32)
    lo = np.maximum(0, np.floor(s / scale).astype(np.int64) - 2)
    hi = np.minimum(n_out - 1, np.ceil((s + np.float32(1)) / scale).astype(np.int64) + 2)
    return lo, hi


def window_misses(n_out):
    """All n_in < n_out at once: the (n_in, destination) pairs whose destination lies outside its source's candidate window."""
    n_in = np.arange(1, n_out, dtype=np.int64)[:, None]
    scale = n_in.astype(np.float32) / np.float32(n_out)
    dst = np.arange(n_out, dtype=np.int64)[None, :]
    src = np.minimum(np.floor(dst.astype(np.float32) * scale).astype(np.int64), n_in - 1)
    s = src.astype(np.float32)
    lo = np.maximum(0, np.floor(s / scale).astype(np.int64) - 2)
    hi = np.minimum(n_out - 1, np.ceil((s + np.float32(1)) / scale).astype(np.int64) + 2)
    bad = (dst < lo) | (dst > hi)
    return [(int(i) + 1, int(d)) for i, d in zip(*np.nonzero(bad))]


def pairs(c):
    """[(level, H, TH, W, TW)] of every top-down add: level i reads level i + 1."""
    return [(i, c.sizes[i][0], c.sizes[i + 1][0], c.sizes[i][1], c.sizes[i + 1][1]) for i in range(n_levels(c) - 1)]


# ------------------------------------------------------------------------------------------------------------------------------
# one predicate per item the lattice claims to reach (csrc/conv_plan.h: conv1x1_to16_top_matches, conv16_matches)
# ------------------------------------------------------------------------------------------------------------------------------
def fused_lateral(c, i):
    """Level i's lateral with a top-down add takes conv1x1_to16_kernel<C, true>."""
    return i < n_levels(c) - 1 and c.out == 16 and c.in_ch[i] in (3, 6)


def thin_wgrad_with_bias(c, i):
    """Level i's 1x1 weight gradient carries the bias gradient as a virtual input channel (conv1x1_to16_top_matches)."""
    return c.out == 16 and c.in_ch[i] in (3, 6)


def fused_embedding(c):
    return c.out == 16


def float_rule_on_fused_lateral(c):
    return any(fused_lateral(c, i) and (rule_differs(H, TH) or rule_differs(W, TW)) for i, H, TH, W, TW in pairs(c))


def float_rule_on_generic_lateral(c):
    return any(not fused_lateral(c, i) and (rule_differs(H, TH) or rule_differs(W, TW)) for i, H, TH, W, TW in pairs(c))


def g_prev_chain(c):
    """Levels the running gradient of the backward is handed through."""
    return n_levels(c)


def top_is_one_pixel(c):
    return n_levels(c) > 1 and c.sizes[-1] == (1, 1)


def fused_c3(c):
    return fused_lateral(c, 0) and c.in_ch[0] == 3


def fused_c6(c):
    return fused_lateral(c, 0) and c.in_ch[0] == 6


def same_size_both(c):
    return any(H == TH and W == TW for _, H, TH, W, TW in pairs(c))


def same_height_only(c):
    return any(H == TH and W != TW for _, H, TH, W, TW in pairs(c))


def one_level(c):
    return n_levels(c) == 1


def wide_neck(c):
    return c.out > 16


def narrow_neck(c):
    return c.out < 16


def ragged_conv16_tiles(c):
    """conv16 maps of several tiles with a ragged last tile column and with a ragged last tile row."""
    return fused_embedding(c) and any(w > T16W and w % T16W != 0 for _, w in c.sizes) and \
        any(h > T16H and h % T16H != 0 for h, _ in c.sizes)


PREDICATES = (float_rule_on_fused_lateral, float_rule_on_generic_lateral, top_is_one_pixel, fused_c3, fused_c6, same_size_both,
              same_height_only, one_level, wide_neck, narrow_neck, ragged_conv16_tiles)


# ------------------------------------------------------------------------------------------------------------------------------
# cotangent sets and which inputs need a gradient
# ------------------------------------------------------------------------------------------------------------------------------
def cot_sets(c):
    """Which outputs get a cotangent: all; the top level only; level 0 only; all but the middle level."""
    n = n_levels(c)
    sets = OrderedDict(all=tuple(range(n)))
    if n > 1:
        sets["top"] = (n - 1,)
        sets["level0"] = (0,)
    if n > 2:
        sets["no-mid"] = tuple(i for i in range(n) if i != n // 2)
    return sets


NEEDS = ("all", "params-only", "not-level0")      # which inputs require a gradient


def x_needs(c, needs):
    n = n_levels(c)
    return {"all": [True] * n, "params-only": [False] * n, "not-level0": [False] + [True] * (n - 1)}[needs]


def zero_grads(c, levels):
    """Names ("x<i>" for the inputs) whose gradient is exactly zero with cotangents on `levels`: the 3x3 conv of an unused level;
    the lateral and the input of a level below every used one (the top-down path runs from level i + 1 to level i only)."""
    out = set()
    for i in range(n_levels(c)):
        if i not in levels:
            out |= {f"fpn.layer_blocks.{i}.0.weight", f"fpn.layer_blocks.{i}.0.bias"}
        if i < min(levels):
            out |= {f"fpn.inner_blocks.{i}.0.weight", f"fpn.inner_blocks.{i}.0.bias", f"x{i}"}
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# inputs, parameters, evaluation
# ------------------------------------------------------------------------------------------------------------------------------
def drawn(c):
    """(fp32 state dict of the module, [fp32 inputs NHWC], [fp32 cotangents NHWC]): the module's own initialisation plus a
    0.02 normal perturbation, biases 0.1 normal; inputs and cotangents standard normal."""
    from dpft_amd.models.necks.fpn import FPN
    g = torch.Generator().manual_seed(c.seed)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(c.seed)
        neck = FPN(list(c.in_ch), c.out)
    sd = OrderedDict()
    for k, v in neck.state_dict().items():
        v = v.detach().clone().contiguous()
        sd[k] = v + torch.randn(v.shape, generator=g) * (0.02 if k.endswith("weight") else 0.1)
    xs = [torch.randn(s, generator=g) for s in level_shapes(c)]
    cots = [torch.randn(s, generator=g) for s in out_shapes(c)]
    return sd, xs, cots


def embedding_kwargs(c):
    return dict(num_feats=c.out, normalize=True)


def evaluate(c, sd32, xs, cots, dtype):
    """One evaluation of the oracle in `dtype` -> dict(outs [NHWC, embedded], neck [NHWC, before the embedding], grads {cot set:
    {name: tensor}}); the inputs' gradients under "x<i>".  A gradient autograd does not produce is an exact zero."""
    sd = {f"{P}.{k}": v.to(dtype).clone().requires_grad_(True) for k, v in sd32.items()}
    feats = OrderedDict((str(i), x.to(dtype).clone().requires_grad_(True)) for i, x in enumerate(xs))
    neck = list(O.fpn(feats, sd, P).values())
    outs = [O.sinusoidal_embedding(v, **embedding_kwargs(c)) for v in neck]
    names = list(sd32) + [f"x{i}" for i in range(len(xs))]
    leaves = [sd[f"{P}.{k}"] for k in sd32] + list(feats.values())
    grads = OrderedDict()
    for key, levels in cot_sets(c).items():
        loss = sum((outs[i] * cots[i].to(dtype)).sum() for i in levels)
        gs = torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)
        grads[key] = {n: (torch.zeros_like(l) if g is None else g).detach() for n, l, g in zip(names, leaves, gs)}
    return dict(outs=[v.detach() for v in outs], neck=[v.detach() for v in neck], grads=grads)


_CACHE = {}


def cached(c):
    """(fp32 state dict, fp32 inputs, fp32 cotangents, fp64 evaluation, fp32 evaluation) of a case; computed once and left
    unchanged."""
    if c.name not in _CACHE:
        sd, xs, cots = drawn(c)
        _CACHE[c.name] = (sd, xs, cots, evaluate(c, sd, xs, cots, torch.float64), evaluate(c, sd, xs, cots, torch.float32))
    return _CACHE[c.name]


def module(c, channel_last=True):
    """A fresh FPN holding the case's state (CPU)."""
    from dpft_amd.models.necks.fpn import FPN
    neck = FPN(list(c.in_ch), c.out, channel_last=channel_last)
    neck.load_state_dict(cached(c)[0])
    for m in neck.modules():                # (load_state_dict copies into the channels-last weights: the layout stays)
        if isinstance(m, torch.nn.Conv2d):
            assert m.weight.permute(0, 2, 3, 1).is_contiguous()
    return neck


def embedding(c):
    from dpft_amd.models.embeddings.sinusoidal import MultiLevelSinusoidalEmbedding
    return MultiLevelSinusoidalEmbedding(n_levels=n_levels(c), **embedding_kwargs(c))


def rel_l2(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).norm() / (ref.norm() + 1e-30))


def rel_max(a, ref):
    """Largest element-wise error over the largest reference magnitude."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / (ref.abs().max() + 1e-30))


# ------------------------------------------------------------------------------------------------------------------------------
# the kernel-level case: the fused lateral above one step of conv1x1_to16_kernel's grid-stride loop
# ------------------------------------------------------------------------------------------------------------------------------
def kernel_case():
    """-> dict(x (B,H,W,C), top (B,TH,TW,K), w (K,1,1,C), b (K,), ref64 (B,H,W,K), ref32) of KERNEL_CASE: the fp64 (and fp32)
    lateral + bias + top gathered by the float index rule."""
    k = KERNEL_CASE
    g = torch.Generator().manual_seed(11)
    x = torch.randn(k["B"], k["H"], k["W"], k["C"], generator=g)
    top = torch.randn(k["B"], k["TH"], k["TW"], k["K"], generator=g)
    w = torch.randn(k["K"], 1, 1, k["C"], generator=g) * 0.5
    b = torch.randn(k["K"], generator=g) * 0.1
    return dict(x=x, top=top, w=w, b=b, ref64=lateral_reference(x, top, w, b, torch.float64),
                ref32=lateral_reference(x, top, w, b, torch.float32))


def lateral_reference(x, top, w, b, dtype):
    H, W, TH, TW = x.shape[1], x.shape[2], top.shape[1], top.shape[2]
    ih, iw = torch.from_numpy(float_src(H, TH)), torch.from_numpy(float_src(W, TW))
    lat = x.to(dtype) @ w.to(dtype).reshape(w.shape[0], -1).t() + b.to(dtype)
    return lat + top.to(dtype)[:, ih][:, :, iw]


def report(c):
    sd, xs, cots, e64, e32 = cached(c)
    e_out = max(rel_l2(a, b) for a, b in zip(e32["outs"], e64["outs"]))
    m_out = max(rel_max(a, b) for a, b in zip(e32["outs"], e64["outs"]))
    live = [(s, k) for s, gs in e64["grads"].items() for k, g in gs.items() if float(g.norm()) > 0]
    e_grad = max(rel_l2(e32["grads"][s][k], e64["grads"][s][k]) for s, k in live)
    m_grad = max(rel_max(e32["grads"][s][k], e64["grads"][s][k]) for s, k in live)
    return (f"{c.name:19s} e32 outputs rel-L2 {e_out:.1e} max {m_out:.1e}   gradients rel-L2 {e_grad:.1e} max {m_grad:.1e}"
            f"   cotangent sets {list(cot_sets(c))}")


if __name__ == "__main__":
    for c in CASES:
        print(f"{c.name:19s} {c.in_ch} -> {c.out}  B {c.B}  {c.sizes}  reaches {[p.__name__ for p in PREDICATES if p(c)]}")
        for i, H, TH, W, TW in pairs(c):
            for n_out, n_in in ((H, TH), (W, TW)):
                for d in rule_differs(n_out, n_in):
                    print(f"    level {i}: {n_out} -> {n_in}  destination {d} reads {float_src(n_out, n_in)[d]} (exact {exact_src(n_out, n_in)[d]})")
    for c in CASES:
        print(report(c))
