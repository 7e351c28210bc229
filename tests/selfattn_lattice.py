"""TEST INFRASTRUCTURE -- the tile lattice of tests/test_selfattn_lattice.py (CPU) and tests/test_gpu_selfattn_tiles.py (GPU).

The fused training self-attention of dpft_amd/csrc/decoder_train.hip (sa_train_fwd_kernel<QW>, sa_train_bwd_q_kernel<QW>,
sa_train_bwd_kv_kernel<KW>) is compiled in seven forms, QW / KW in {1, 2, 3, 4, 5, 6, 8} queries / keys per wave, and the host
picks one per launch from (B, Q, V) so that each grid is one round of at most 256 blocks.  At the model's Q = 400, V = 3 every
batch size from 1 to 6 runs a different form.  The lattice puts each form in front of the fp64 oracle, at sizes chosen for what
goes wrong in such kernels:

  * a ragged last tile (Q % (4 QW) != 0) in every form from 2 up: rows >= Q are loaded clamped to Q - 1 and must add nothing to
    dx / dxp or to the parameter-gradient atomics, and must write nothing;
  * the key loop  k = slice; k < Q; k += 16  with keys k and k + 8 under one mask hash: Q % 16 in 1..8 (no second key in the
    whole last group), in 9..15 (second key for some slices only), 0 (control), Q < 8 (whole slices empty: max = -inf, den = 0,
    the merge must drop them) and Q = 1 (softmax over one key);
  * more than 64 KB of dynamic LDS in all three kernels (the hipFuncSetAttribute branch of the dispatch);
  * x as the (Q, 16) query table broadcast over the batch with stride 0 (the first decoder layer on every step);
  * logits above 100, where a lost max subtraction or a wrong correction factor in the slice merge overflows fp32.

No GPU code here: the case table, a restatement of the host rule and of the three LDS formulas (compared with
dpft_selfattn_train_tiles, which answers from the code the launches use), the operands, and the reference -- oracle mha + residual
+ LayerNorm with the kernels' dropout decisions replayed (tests/dropout_masks.py) -- in fp64 and, as the yardstick of the
large-logit case, in fp32.  ``python -m tests.selfattn_lattice`` prints the table."""
import os
from collections import namedtuple

import torch

NUM_CU = 256                      # common.h: kNumCU
FORMS = (1, 2, 3, 4, 5, 6, 8)     # the compiled QW / KW
KERNELS = ("fwd", "bwd_q", "bwd_kv")
ENV = ("DPFT_SA_QW_FWD", "DPFT_SA_QW_BWD", "DPFT_SA_KW")      # tuning variables, one per kernel
TC, TH = 16, 8                    # channels, heads
LDS_DEFAULT = 64 * 1024           # above it the dispatch raises the kernel's dynamic LDS limit

Case = namedtuple("Case", "name V B Q qw table logit_scale why")

# name, V, B, Q, expected QW = KW, x is the (Q, 16) table, scale of the in_proj q / k rows
CASES = [
    Case("one-key", 1, 1, 1, 1, False, 1.0, "single key; q/k-path gradients are exactly 0 in the reference"),
    Case("empty-slices", 2, 1, 7, 1, False, 1.0, "Q < 8: slice 7 never runs; 7 % 4 = 3 ragged"),
    Case("qw2", 4, 16, 29, 2, False, 1.0, "29 % 8 = 5 ragged; 29 % 16 = 13"),
    Case("qw3", 4, 16, 41, 3, False, 1.0, "41 % 12 = 5; 41 % 16 = 9: only slice 0 has a second key in the last group"),
    Case("qw4", 4, 16, 56, 4, False, 1.0, "56 % 16 = 8: last group has no second key at all; ragged tile"),
    Case("qw5-ragged", 4, 32, 33, 5, False, 1.0, "33 % 20 = 13; 33 % 16 = 1"),
    Case("qw6", 4, 32, 47, 6, False, 1.0, "47 % 24 = 23; 47 % 16 = 15"),
    Case("qw7to8", 4, 64, 26, 8, False, 1.0, "the 7 -> 8 mapping; one tile, 26 of 32 rows live"),
    Case("qw8-exact", 4, 64, 64, 8, False, 1.0, "two full tiles, Q % 16 = 0: control without edges"),
    Case("lds-160k", 3, 8, 400, 8, False, 1.0, "all three kernels request > 64 KB of LDS; 400 % 32 = 16"),
    Case("table", 3, 4, 24, 1, True, 1.0, "x is the (Q, 16) table with batch = 4 (stride 0); its gradient summed over views and batch"),
    Case("L", 2, 2, 40, 1, False, 8.0, "in_proj q / k rows times 8: |scaled score| > 100, maxima outside the first key slice"),
]
SEED_HIGH, SEED_NEG = (12345678901234, 7), (-5, 1)      # (seed, salt): above 2^32, and negative


def by_name(name):
    return next(c for c in CASES if c.name == name)


def runs(c):
    """[(p_drop, seed, salt)] of a case: p = 0 everywhere; p = 0.25 with the two seeds alternating over the table, except
    one-key (its only key dropped leaves nothing to compare) and lds-160k, which runs once more at p = 0.1."""
    out = [(0.0, 0, 3)]
    if c.name == "lds-160k":
        out.append((0.1,) + SEED_HIGH)
    elif c.name != "one-key":
        out.append((0.25,) + (SEED_HIGH, SEED_NEG)[CASES.index(c) % 2])
    return out


RUNS = [(c, r) for c in CASES for r in runs(c)]


def run_id(cr):
    c, (p, seed, _) = cr
    return c.name if p == 0 else f"{c.name}-p{p}-seed{'neg' if seed < 0 else 'high'}"


# ---------------------------------------------------------------------------------------------------------------------
# the host rule of decoder_train.hip (pick_qw, sa_tiles), restated
# ---------------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def raw_qw(B, Q, V):
    """Queries per wave before 7 is mapped to 8: Q split over the tiles that fit one round of the chip, four waves a block."""
    tiles = max(1, NUM_CU // (V * B))
    return min(8, max(1, cdiv(cdiv(Q, tiles), 4)))


def pick_qw(B, Q, V, which=0, env=None):
    env = os.environ if env is None else env
    try:
        forced = int(env.get(ENV[which], "0") or "0")
    except ValueError:
        forced = 0
    if 1 <= forced <= 8 and forced != 7:
        return forced
    qw = raw_qw(B, Q, V)
    return 8 if qw == 7 else qw


def lds_bytes(Q, qw):
    """Dynamic LDS of (fwd, bwd_q, bwd_kv) for their (QW, QW, KW)."""
    common = 48 * 16 + 48                                   # in_proj rows + bias
    qf, qq, kt = (4 * w for w in qw)
    return (4 * (Q * 32 + common + qf * TC + qf * TH * 8 * 4),          # K, V | Q' tile | (max, den, o0, o1) per (query, head, slice)
            4 * (Q * 32 + common + 6 * qq * TC + qq * TH + 2 * qq * TC),  # K, V | six tiles | delta | LayerNorm partials
            4 * (Q * 48 + common + 6 * kt * TC))                        # Q', dA of all queries, lse, delta | six tiles


def tiles(B, Q, V, env=None):
    """-> ((qw_fwd, qw_bwd_q, kw), (lds_fwd, lds_bwd_q, lds_bwd_kv)): what dpft_selfattn_train_tiles must answer."""
    qw = tuple(pick_qw(B, Q, V, w, env) for w in range(3))
    return qw, lds_bytes(Q, qw)


def library_tiles(B, Q, V):
    """The same from the library (host code: no GPU needed)."""
    import ctypes as C
    from dpft_amd.hip.lib import lib
    qw, lds = (C.c_int32 * 3)(), (C.c_int64 * 3)()
    lib.call("dpft_selfattn_train_tiles", B, Q, V, C.byref(qw), C.byref(lds))
    return tuple(qw), tuple(lds)


def ragged(c):
    return c.Q % (4 * c.qw) != 0


def key_class(Q):
    """Class of the key loop's last 16-key group."""
    if Q < 8:
        return "Q<8"
    r = Q % 16
    return "0" if r == 0 else ("1..8" if r <= 8 else "9..15")


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
def make_layers(c):
    """V MLFusion layers on the CPU, initialised like the self-attention tests of tests/test_gpu_kernels.py (non-trivial
    biases, norm weights around 1); case L scales the q / k rows of in_proj (weight and bias)."""
    from dpft_amd.models.fusers.mpfusion import MLFusion
    torch.manual_seed(5)
    layers = [MLFusion(d_model=16, d_ffn=32, n_levels=2, n_heads=8, n_points=2, activation="Mish", dropout=0.0, norm=True)
              for _ in range(c.V)]
    for ml in layers:
        for p in ml.parameters():
            if p.dim() == 1:
                torch.nn.init.normal_(p, 0.0 if p is not ml.norm1.weight else 1.0, 0.3)
        if c.logit_scale != 1.0:
            with torch.no_grad():
                ml.self_attn.in_proj_weight[:32] *= c.logit_scale
                ml.self_attn.in_proj_bias[:32] *= c.logit_scale
    return layers


def operands(c):
    """fp32 CPU tensors: x (B,Q,16) -- (Q,16) for the table case --, pos (Q,16), gy (V,B,Q,16) the cotangent."""
    g = torch.Generator().manual_seed(7919 * (1 + CASES.index(c)))
    x = torch.randn((c.Q, 16) if c.table else (c.B, c.Q, 16), generator=g) * 0.7
    pos = torch.randn(c.Q, 16, generator=g) * 0.5
    gy = torch.randn(c.V, c.B, c.Q, 16, generator=g)
    return x, pos, gy


PARAM_KEYS = ("ml.self_attn.in_proj_weight", "ml.self_attn.in_proj_bias", "ml.self_attn.out_proj.weight",
              "ml.self_attn.out_proj.bias", "ml.norm1.weight", "ml.norm1.bias")      # the order of train_fused.sa_params
GRAD_NAMES = ("in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b", "norm1_w", "norm1_b")


def grad_names(c):
    return ["x", "pos"] + [f"v{v}.{n}" for v in range(c.V) for n in GRAD_NAMES]


# ---------------------------------------------------------------------------------------------------------------------
# the reference: oracle mha + dropout1 + residual + LayerNorm with the kernels' masks, fp64 (or fp32: case L's yardstick)
# ---------------------------------------------------------------------------------------------------------------------
def reference(c, layers, x, pos, gy, run, dtype=torch.float64):
    """-> (y (V,B,Q,16), [dx, dpos, six parameter gradients per view]) in ``dtype`` on the CPU, one view at a time (the
    attention matrix and its masks are (B,8,Q,Q) per view: the largest case stays within a few hundred MB)."""
    from oracle import dprt_oracle as O
    from tests.dropout_masks import self_attn_masks
    p_drop, seed, salt = run
    xl = x.detach().to(dtype).requires_grad_(True)
    posl = pos.detach().to(dtype).requires_grad_(True)
    ys, pgrads = [], []
    dx, dpos = torch.zeros_like(xl), torch.zeros_like(posl)
    for v, ml in enumerate(layers):
        sd = {f"ml.{k}": t.detach().to(dtype).cpu().requires_grad_(True) for k, t in ml.state_dict().items()
              if k.startswith(("self_attn.", "norm1."))}
        xb = xl.unsqueeze(0).expand(c.B, -1, -1) if c.table else xl
        qk = xb + posl.unsqueeze(0)
        if p_drop > 0:
            att, d1 = self_attn_masks(seed, salt, p_drop, 1, c.B, c.Q, view0=v)
            att, d1 = torch.from_numpy(att[0]).to(dtype), torch.from_numpy(d1[0]).to(dtype)
            sa = O.mha(qk, qk, xb, sd, "ml.self_attn", TH, att_scale=att) * d1
        else:
            sa = O.mha(qk, qk, xb, sd, "ml.self_attn", TH)
        y = O._ln(xb + sa, sd, "ml.norm1")
        g = torch.autograd.grad(y, [xl, posl] + [sd[k] for k in PARAM_KEYS], gy[v].to(dtype))
        dx += g[0]
        dpos += g[1]
        pgrads += list(g[2:])
        ys.append(y.detach())
    return torch.stack(ys), [dx, dpos] + pgrads


def scaled_scores(c, layers, x, pos):
    """fp64 scaled scores q k^T / sqrt(2) of every view: (V,B,8,Q,Q)."""
    out = []
    xb = (x.unsqueeze(0).expand(c.B, -1, -1) if c.table else x).double()
    qk = xb + pos.double().unsqueeze(0)
    for ml in layers:
        w, b = ml.self_attn.in_proj_weight.detach().double(), ml.self_attn.in_proj_bias.detach().double()
        q = (qk @ w[:16].T + b[:16]).view(c.B, c.Q, TH, 2).transpose(1, 2)
        k = (qk @ w[16:32].T + b[16:32]).view(c.B, c.Q, TH, 2).transpose(1, 2)
        out.append(q @ k.transpose(-1, -2) / 2 ** 0.5)
    return torch.stack(out)


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def table_rows(from_library=False):
    rows = []
    for c in CASES:
        qw, lds = library_tiles(c.B, c.Q, c.V) if from_library else tiles(c.B, c.Q, c.V)
        rows.append(f"{c.name:13s} V={c.V} B={c.B:2d} Q={c.Q:3d}  QW fwd/bwd_q/bwd_kv {qw[0]}/{qw[1]}/{qw[2]} (rule before 7->8: "
                    f"{raw_qw(c.B, c.Q, c.V)})  LDS bytes {lds[0]:6d}/{lds[1]:6d}/{lds[2]:6d}  Q%(4QW)={c.Q % (4 * c.qw):2d} "
                    f"Q%16={c.Q % 16:2d}  runs p={[r[0] for r in runs(c)]}")
    return rows


if __name__ == "__main__":
    print("\n".join(table_rows()))
    try:
        lib_rows = table_rows(from_library=True)
    except Exception as e:      # the library is not built: the restatement alone
        print("library not asked:", e)
    else:
        print("library agrees" if lib_rows == table_rows() else "LIBRARY DIFFERS:\n" + "\n".join(lib_rows))
