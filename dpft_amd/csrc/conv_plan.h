// What a convolution launch will be, decided once: pure host functions of the descriptor, the compute mode (conv.hip's, passed in
// as PlanMode) and the tuning switches.  conv.hip's entries launch what a plan names; its sizing queries read the same plans.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/dpft_hip.h"
#include "host_consts.h"

namespace dpft {

constexpr int BK = 32;        // generic path K-step
constexpr int BKV = 64;       // vector path K-step: one barrier pair per 2048+ MFMA cycles, and the register
                              // prefetch of the next step has that long to land (HBM/L2 latency under load)
constexpr int BKP = 64;       // wgrad vector path: pixels per step
constexpr int T16H = 8, T16W = 32;          // conv16 kernels: output tile of a workgroup
constexpr int STEM_OH = 4, STEM_OW = 16;    // stem weight gradient: output tile of a workgroup
constexpr int kBiasBlocks = 256;            // bias_grad_slab_kernel: blocks (= partial-sum rows) at most
constexpr int kConv16Slab = 2320;           // conv16 weight gradient: floats per block slab (2304 + 16 bias column sums)

// Workspace layout (round 4): [ticket header: kWsHeader bytes][split-K partial slabs].  The header holds one int per output
// tile of a split-K launch (IgemmArgs::sk_ticket); it must be ZERO when a buffer is first handed to the library
// (dpft_conv2d_workspace_init) and every launch leaves it zero again.
constexpr size_t kWsHeader = 16384;
constexpr int kWsTickets = (int)(kWsHeader / sizeof(int));

// kernel family of a conv launch (dpft_profile_get_family; bench.py prices each against ITS pipe's peak):
//   0 fp32 MFMA (v_mfma_f32_32x32x2_f32: igemm_pipe / igemm_vec / wgrad_pipe / wgrad_vec), 1 three-term bf16 split, six
//   v_mfma_f32_32x32x16_bf16 per fp32 product (conv_x3.hip), 2 bf16 operands on the bf16 MFMA (mixed precision),
//   3 no matrix core: thin-channel / 16-channel / generic vector-ALU kernels
enum { kFamF32 = 0, kFamX3 = 1, kFamBf16 = 2, kFamVector = 3 };

// compute: 0 fp32 MFMA, 1 bf16 operands, 2 3 x bf16 split; split_on: the big multi-tap GEMMs take the split kernels (2, or 0 + split switch)
struct PlanMode { int compute; bool split_on; };

// Every DPFT_* switch of conv.hip's host code, parsed once on first use (DPFT_FORCE_TILE / DPFT_FORCE_WGRAD / DPFT_X3_ROW3: live, once per plan)
struct ConvTuning {
    static int env(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
    static int compute_env() { const char* e = getenv("DPFT_CONV_COMPUTE"); return !e ? 0 : (!strcmp(e, "bf16") ? 1 : (!strcmp(e, "bf16x3") ? 2 : 0)); }
    int compute0 = compute_env();                        // DPFT_CONV_COMPUTE=fp32|bf16|bf16x3 presets the compute mode (tests, sweeps)
    int split0 = env("DPFT_CONV_SPLIT", 1) != 0;         // DPFT_CONV_SPLIT=0 presets the split switch off: fp32 MFMA everywhere
    int sk_fixup = env("DPFT_SK_FIXUP", 7);              // in-kernel split-K fix-up, bits: 1 forward, 2 data gradient, 4 residual data gradient; 0: the separate reduction kernels (A/B switch)
    int x3_1x1_mink = env("DPFT_X3_1X1_MINK", 0);        // tuning aid (0 = off): 1x1 stride-1 convs reducing over at least this many channels take the split kernels (see choose_tile)
    int x3_narrow = env("DPFT_X3_NARROW", 2);            // split kernels: 128 x 64 tiles where the K split would exceed this; 0 off (see choose_tile)
    bool shortk_tile = env("DPFT_SHORTK_TILE", 1) != 0;  // A/B switch: 128 x 64 tiles for short reductions over many row tiles (see choose_tile)
    const char* tile_eff = getenv("DPFT_TILE_EFF");      // tuning aid: "e128x128,e128x64,e64x64[,max row tiles it applies to]"
    int split_below = env("DPFT_SPLIT_BELOW", kNumCU);   // tuning aid: split K below this many workgroups (see choose_tile)
    int b16w = env("DPFT_B16W", 2);                      // 256-row bf16 tiles: 0 off | 1 forward + data gradients | 2 forward only (see big16_tile)
    int b16w_min256 = env("DPFT_B16W_MIN256", 100);      // fewest 256 x 256 tiles that take them
    int b16w_min128 = env("DPFT_B16W_MIN128", 1 << 30);  // 256 x 128 tiles: measured at par or behind the four-wave kernels (profiles/r06_b16w_*.txt): off
    int b16w_split = env("DPFT_B16W_SPLIT", 4);          // tuning aid: largest K split of the 256 x 128 tiles
    int pipe = env("DPFT_PIPE", 3);                      // software-pipelined kernels (conv_pipe.h), bit 0: igemm, bit 1: wgrad; 0 keeps igemm_vec / wgrad_vec (A/B measurements)
    bool x3_all = env("DPFT_X3_ALL", 0) != 0;            // tuning aid: compute mode 2 sends the 1x1 convs to the split kernels too
    int shortk = env("DPFT_SHORTK", 0);                  // tuning aid: 64 x 64 pipelined tiles with Ktot <= this take 32-wide K-steps (32 KB of LDS)
    int ksplit = env("DPFT_KSPLIT", -1);                 // tuning aid: 0 / 1 force the 512-thread K-split form of igemm_vec off / on
    bool wgrad16_tiled = env("DPFT_WGRAD16_TILED", 1) != 0;      // A/B switch: LDS-tiled conv16 weight gradient
    bool wgrad_stem = env("DPFT_WGRAD_STEM", 1) != 0;    // A/B switch: LDS-tiled stem weight gradient
    const char* skip = skip_families();                  // timing experiments: families whose launches are skipped (see skip_family)
    bool thin_fwd = env("DPFT_THIN_FWD", 1) != 0;        // A/B switch: streaming 1x1 -> 16 forward
    bool bnact_fixup = env("DPFT_BNACT_FIXUP", 1) != 0;  // A/B switch: inference epilogue in the fix-up of every split vector launch
    int epf = env("DPFT_EPF", 7);                        // epilogue-operand prefetch, bits: 1 residual data gradient, 2 data gradient with a BatchNorm reduction, 4 inference residual; 0: plain epilogues (A/B switch)
    bool fpn_fuse = env("DPFT_FPN_FUSE", 1) != 0;        // A/B switch: top-down add / positional embedding in the FPN convs' epilogues
    bool wgrad16_pipe = env("DPFT_WGRAD16_PIPE", 1) != 0;        // A/B switch: LDS-DMA weight gradient on bf16 tensors
    bool wgrad_x3 = env("DPFT_WGRAD_X3", 1) != 0;        // A/B switch: big weight gradients on the split kernels
    bool wgrad_x3_1x1 = env("DPFT_WGRAD_X3_1X1", 1) != 0;        // A/B switch: ... the 1x1 ones too
    bool bias_slab = env("DPFT_BIAS_SLAB", 1) != 0;      // A/B switch: bias gradient through workspace slabs
    bool bias_fuse = env("DPFT_BIAS_FUSE", 1) != 0;      // A/B switch: bias gradient inside the thin weight-gradient kernels
};
inline const ConvTuning& tuning() { static const ConvTuning t; return t; }

// DPFT_SKIP=family,... (timing experiments, wrong results; README.md): fwd3x3 fwd1x1 dgrad3x3 dgrad1x1 (from 4096 rows on) wgrad wreduce
inline bool skip_family(const char* family) { return tuning().skip && strstr(tuning().skip, family); }      // "wgrad", "wreduce"
inline bool skip_conv(const char* fam3x3, const char* fam1x1, int kh, int64_t rows) {      // "fwd3x3" / "fwd1x1", "dgrad3x3" / "dgrad1x1"
    return rows >= 4096 && ((kh == 3 && skip_family(fam3x3)) || (kh == 1 && skip_family(fam1x1)));
}

struct ForceTile {      // DPFT_FORCE_TILE="bm,bn,splits" (tuning aid, tests): read live, once per plan
    int bm = 0, bn = 0, splits = 0;
    const char* env = getenv("DPFT_FORCE_TILE");
    bool set = env != nullptr, ok = env && sscanf(env, "%d,%d,%d", &bm, &bn, &splits) == 3;
};

// ---- which shapes the kernels outside the implicit GEMM take (conv16_kernels.h, conv_stream.hip) -------------------
bool stream1x1_match(const dpft_conv_desc* d, int* tile_rows);      // conv_stream.hip (its own switches)
inline bool conv16_matches(const dpft_conv_desc* d) {
    return d->C == 16 && d->K == 16 && d->kh == 3 && d->kw == 3 && d->stride == 1 && d->pad == 1;
}
inline bool wgrad_stem7_matches(const dpft_conv_desc* d) {
    // (each block ends with a 3-round wave reduction and a 37 KB slab: worth it from ~8 tiles per block on -- the radar stems,
    // 27 k output pixels, stay with the generic kernel: 26.6 vs 37.0 us)
    return d->kh == 7 && d->kw == 7 && d->stride == 2 && d->pad == 3 && d->C == 3 && d->K == 64 && !d->act16 &&
           (int64_t)d->B * d->OH * d->OW >= 131072;
}
// the lateral of a raw-input level with the top-down add in its epilogue (any map size: it replaces two launches)
inline bool conv1x1_to16_top_matches(const dpft_conv_desc* d) {
    return d->kh == 1 && d->kw == 1 && d->stride == 1 && d->pad == 0 && d->K == 16 && (d->C == 3 || d->C == 6) && !d->act16;
}
inline bool conv1x1_to16_matches(const dpft_conv_desc* d) {
    // (below ~256 k pixels the launch is latency-sized and the generic path is as fast: radar laterals 13.1 vs 14.6 us)
    return conv1x1_to16_top_matches(d) && (int64_t)d->B * d->H * d->W >= 262144;
}
inline int conv16_wgrad_blocks(const dpft_conv_desc* d) {      // streaming form; also the workspace bound of both forms
    const long groups = (long)d->B * d->H * cdiv(d->W, 4);
    return (int)std::max<long>(1, std::min<long>(kNumCU * 4, groups / 64));
}
inline int conv16_wgrad_tiled_blocks(const dpft_conv_desc* d) {
    const long tiles = (long)d->B * cdiv(d->H, T16H) * cdiv(d->W, T16W);
    return (int)std::max<long>(1, std::min<long>(std::min<long>(kNumCU * 4, conv16_wgrad_blocks(d)), tiles));
}

// ---- the implicit GEMM of a forward conv / data gradient -----------------------------------------------------------
struct GemmDims { int M, N, C, Ktot, ksteps; int64_t in_elems; };      // Y[M][N] = A[M][Ktot] * W^T; C = channels of the A-source tensor, in_elems = its size
inline GemmDims gemm_dims(const dpft_conv_desc* d, bool dgrad) {
    GemmDims g;
    g.C = dgrad ? d->K : d->C; g.N = dgrad ? d->C : d->K;
    g.M = dgrad ? d->B * d->H * d->W : d->B * d->OH * d->OW;
    g.in_elems = dgrad ? (int64_t)d->B * d->OH * d->OW * d->K : (int64_t)d->B * d->H * d->W * d->C;
    g.Ktot = d->kh * d->kw * g.C;
    g.ksteps = (g.C % BKV) == 0 ? g.Ktot / BKV : cdiv(g.Ktot, BK);
    return g;
}

struct TileChoice { int bm, bn, splits; bool vec, x3 = false; };      // x3: chosen for the 3 x bf16 split kernels (compute mode 2, multi-tap filters)

// in-kernel split-K fix-up instead of a reduction launch (never for a parity class of a strided data gradient: those do not split)
inline bool sk_fixup_ok(const GemmDims& g, int splits, int kind) {      // kind: 1 forward, 2 data gradient, 4 residual data gradient
    return (tuning().sk_fixup & kind) && splits > 1 && (g.N & 3) == 0 && (int64_t)splits * g.M * g.N * 4 < (1ll << 31);
}

// `taps` = kh * kw of the problem (1 = unknown / not asked): in compute mode 2 the filters with more than one tap -- the
// deep reductions -- take the 3 x bf16 split kernels (conv_x3.hip), whose best tiles differ: their operand stream
// (6 bytes per element through L2 -> LDS) is what bounds them (tools/x3_abl.sh), so 128 x 128 tiles with a K split
// that brings the grid to about one workgroup per CU; the 1x1 convs stay on the fp32 MFMA (measured at par there).
inline int taps_of(const dpft_conv_desc* d) { return (d->kh * d->kw == 1 && d->stride == 1) ? -1 : d->kh * d->kw; }
inline TileChoice choose_tile(int M, int N, int C, int ksteps, int taps, const PlanMode& mode, const ForceTile& force) {
    const ConvTuning& tn = tuning();
    TileChoice t;
    t.vec = (C % BKV) == 0;
    t.x3 = false;
    // (only where the GEMM is big enough to be bound by the matrix pipe: the latency-sized problems of the radar encoders
    // measured 2x SLOWER on the 128-row tiles, profiles/r05_x3_table.txt)
    // taps = -1: a 1x1 stride-1 conv on fp32 operands; DPFT_X3_1X1_MINK (tuning aid, 0 = off) sends those with a reduction of at
    // least that many channels to the split kernels too.  Measured in the step (same box, two rounds): off 24.18 / 24.23 ms,
    // >= 1024 channels 24.66 / 24.71, >= 512 24.68 / 24.90, >= 256 27.5 / 25.8 -- the forward loses as well (1.78 -> 1.81 ms per frame)
    const bool deep1x1 = taps == -1 && tn.x3_1x1_mink > 0 && (int64_t)ksteps * BKV >= tn.x3_1x1_mink;
    if (mode.split_on && (taps > 1 || deep1x1) && t.vec && !force.set && 2.0 * M * N * (double)ksteps * BKV >= 2e9) {
        t.x3 = true;
        if (N >= 128) {
            t.bm = 128; t.bn = 128;
            const int64_t nwg = (int64_t)cdiv(M, 128) * cdiv(N, 128);
            int sp = (int)std::max<int64_t>(1, std::min<int64_t>(8, kNumCU / nwg));      // at most one workgroup per CU: one round
            while (sp > 1 && ksteps / sp < 4) --sp;
            // Few row tiles (batch-1 inference: 15 at layer 3; layer 4 in training): a deep K split of 128 x 128 tiles ends in a
            // fix-up over 4-8 slabs of 64 KB read by ONE workgroup per tile -- 128 x 64 tiles reach the same workgroup count with
            // half the split and quarter-size fix-ups: batch-1 forward 3.50 -> 3.10-3.24 ms, training step unchanged
            // (tools/infer_ab.sh; DPFT_X3_NARROW=0 switches it off, =4 moves the threshold)
            if (tn.x3_narrow && sp > tn.x3_narrow) {
                t.bn = 64;
                const int64_t nwg64 = (int64_t)cdiv(M, 128) * cdiv(N, 64);
                sp = (int)std::max<int64_t>(1, std::min<int64_t>(8, kNumCU / nwg64));
                while (sp > 1 && ksteps / sp < 4) --sp;
            }
            t.splits = sp;
            // (measured, round-5 A/B, docs/history: 128 x 64 tiles without the K split -- which would keep the data gradients' epilogue
            // operand prefetch -- lose: layer-3 forward 82 vs 70 us per call, data gradient 70 vs 68.5)
        } else {
            t.bm = 64; t.bn = 64; t.splits = 1;
        }
        return t;
    }
    if (force.ok && t.vec) {
        t.bm = force.bm; t.bn = force.bn; t.splits = force.splits < 1 ? 1 : force.splits;
        while (t.splits > 1 && ksteps / t.splits < 2) --t.splits;      // every split keeps at least one pipelined K-step
        return t;
    }
    if (!t.vec) {
        t.bm = 128;
        t.bn = (N <= 32) ? 32 : 64;
        t.splits = 1;
        return t;
    }
    // candidate tiles ordered by per-flop efficiency; pick the one that fills the chip best
    const int cand[3][2] = {{128, 128}, {128, 64}, {64, 64}};
    double eff[3] = {1.0, 0.92, 0.80};
    // Short reductions over many row tiles (the 1x1 convs of camera layers 1-2, K <= 256): the kernel is its epilogue
    // (statistics / residual / BatchNorm-reduction operands, staged stores), and with 128 x 128 tiles all workgroups of a
    // wave reach it together; 128 x 64 measured 10-25 % faster there (round-3 tile A/B, docs/history: 176 -> 129 us on the
    // 128x228 256<-64 data gradient), not on the 57-row-tile grids of layer 3.
    if (tn.shortk_tile && (int64_t)ksteps * BKV <= 256 && (int64_t)cdiv(M, 128) * cdiv(N, 128) >= 768) {
        eff[0] = 0.88; eff[1] = 1.0; eff[2] = 0.85;
    }
    if (tn.tile_eff) {
        double a0, a1, a2; int rows = 1 << 30;
        if (sscanf(tn.tile_eff, "%lf,%lf,%lf,%d", &a0, &a1, &a2, &rows) >= 3 && cdiv(M, 128) <= rows) { eff[0] = a0; eff[1] = a1; eff[2] = a2; }
    }
    double best = -1;
    t.bm = 64; t.bn = 64;
    for (int i = 0; i < 3; ++i) {
        const int bm = cand[i][0], bn = cand[i][1];
        if (bn > 64 && N <= 64) continue;
        const int64_t nwg = (int64_t)cdiv(M, bm) * cdiv(N, bn);
        const int slots = kNumCU * 2;  // two resident workgroups per CU
        const double waves = (double)nwg / slots;
        const double fill = waves / ceil(waves);
        // padding waste in N and M
        const double pad = ((double)M * N) / ((double)cdiv(M, bm) * bm * (double)cdiv(N, bn) * bn);
        const double score = eff[i] * fill * pad;
        if (score > best) {
            best = score;
            t.bm = bm;
            t.bn = bn;
        }
    }
    // split-K when even the smallest tile leaves most CUs idle (radar branches, layer4)
    const int64_t nwg = (int64_t)cdiv(M, t.bm) * cdiv(N, t.bn);
    t.splits = 1;
    // DPFT_SPLIT_BELOW (tuning aid): the isolated 232-tile layer-4 1x1 forward runs 52.9 us split in three vs 35.9 us
    // unsplit (round-3 tile A/B, docs/history), but over the whole step 128 / 192 / 256 are within run-to-run noise (conv time 28.2 /
    // 27.9 / 28.0 ms): the threshold stays at one workgroup per CU.
    // (round 4) 200 ... 255 tiles with a SHALLOW reduction (<= 32 K-steps: the 1x1 convs of camera layer 4, 232 tiles)
    // stay unsplit: the split's slab round trip + reduction launch cost more than the idle tenth of the chip
    // (round-3 tile A/B, docs/history: 16x29 2048->512 forward 53.7 -> 36.9 us, 512->2048 data gradient 55.1 -> 40.1 us)
    const bool shallow_nearly_full = nwg >= 200 && ksteps <= 32;
    if (nwg < tn.split_below && ksteps >= 8 && !shallow_nearly_full) {
        int s = (int)((kNumCU * 2 + nwg - 1) / nwg);
        s = s > 16 ? 16 : s;
        while (s > 1 && ksteps / s < 4) --s;
        t.splits = s;
    }
    return t;
}

// act16 = 2 (bf16 activations and bf16 weights): the 256-row tiles of conv_b16w.hip (eight waves, 64 x 128 / 64 x 64 outputs
// per wave); the tile may carry a K split (in-launch fix-up).  The tile height must not depend on the workspace:
// dpft_conv2d_stats_tiles answers without one.  Alone, the 256 x 256 tiles win on the wide short-K 1x1 convs (batch 8,
// 256 -> 1024 forward + statistics 30.9 -> 22.7 us, its data gradient 28.0 -> 19.3, 128 -> 512 forward 46.1 -> 35.8) and lose on
// N = 256 problems (57 row tiles: a K split's slab round trip costs more than the idle CUs).  INSIDE the training step the data
// gradients lose -- a 512-thread workgroup that owns a CU's whole LDS cannot share the CU with the weight-gradient stream's
// workgroups the way three 48 KB workgroups do -- but the FORWARD has no weight-gradient stream beside it: bf16 batch 8, same box,
// two rounds: off 22.91 / 22.78 ms, forward only 22.60 / 22.60, forward + data gradients 24.14 / 24.21 (profiles/r06_b16w_*.txt).
// Default: forward only (DPFT_B16W=2); =1 both, =0 off.
inline bool big16_tile(const dpft_conv_desc* d, const GemmDims& g, bool dgrad, bool has_ws, const ForceTile& force, TileChoice& t) {
    const ConvTuning& tn = tuning();
    if (!tn.b16w || d->act16 != 2 || (g.C % BKV) != 0 || (g.N % 128) != 0 || force.set) return false;
    if (tn.b16w == 2 && dgrad) return false;      // 2: forward convs only (no weight-gradient stream beside them)
    if (dgrad && d->stride > 1) return false;      // (parity classes / the all-tap form keep their kernels)
    if (g.in_elems >= (1ll << 29) || (int64_t)g.N * g.Ktot >= (1ll << 29)) return false;
    const int64_t mt = cdiv(g.M, 256);
    if ((g.N % 256) == 0 && mt * (g.N / 256) >= tn.b16w_min256) {
        t.bm = 256; t.bn = 256; t.splits = 1; t.vec = true; t.x3 = false;
        return true;
    }
    const int64_t n128 = mt * (g.N / 128);
    if (n128 >= tn.b16w_min128) {
        t.bm = 256; t.bn = 128; t.vec = true; t.x3 = false;
        int sp = 1;
        if (has_ws && n128 < 200 && tn.b16w_split > 1) {
            sp = (int)std::min<int64_t>(tn.b16w_split, (kNumCU + n128 / 2) / n128);
            while (sp > 1 && g.Ktot / BKV / sp < 8) --sp;
        }
        t.splits = sp < 1 ? 1 : sp;
        return true;
    }
    return false;
}

enum IgemmKind { kFwd, kFwdBnact, kDgrad, kDgradRes, kDgradClass };      // kFwdBnact: forward with the inference epilogue; kDgradClass: one parity class of a strided data gradient
// kStream1x1: conv_stream.hip | kConv16, kThin: conv16_kernels.h | kGeneric: igemm_gen_kernel | kVec, kVecKS2: igemm_vec_kernel (KS = 1, 2)
// | kAllTap: strided data gradient over all taps | kPipe, kPipe16: igemm_pipe_kernel on fp32 / bf16 operands | kB16w: 256-row tiles of
// conv_b16w.hip | kX3Planes, kX3: conv_x3.hip on three bf16 planes / three-term split | kTwoPass (kFwdBnact): plain forward + elementwise
// pass instead | kClasses (kDgrad): one launch per parity class, each planned as kDgradClass
enum IgemmKernel { kStream1x1, kConv16, kThin, kGeneric, kVec, kVecKS2, kAllTap, kPipe, kPipe16, kB16w, kX3Planes, kX3, kTwoPass, kClasses };
enum { kReduceNone, kReducePlain, kReduceStats, kReduceResidual };

struct IgemmIn {      // what the entry knows
    bool ws = false, bias = false, pro = false, pro_relu = false, residual = false, accumulate = false;
    bool stats = false, sums = false;          // statistics wanted; as column sums where the kernel can
    bool planes = false;                       // a_planes and w_planes given
    bool bnr = false, bnr_mask8 = false, res_mask8 = false;      // BatchNorm-reduction operands (bnr: sums given and N % 4 == 0)
    int M = 0, ksteps = 0;                     // kDgradClass: rows and K-steps of the class
};
struct IgemmPlan {
    IgemmKernel kernel = kGeneric;
    int family = kFamVector;
    int bm = 0, bn = 0, splits = 1;      // the tile that runs (after the 64 x 64 overrides); kStream1x1: bm = rows of a workgroup
    int pbk = BKV;                       // K-step the kernel counts ksteps in
    bool fixup = false;                  // split-K: the last workgroup of a tile runs the epilogue (needs `tickets` header slots)
    int reduce = kReduceNone;            // ... or this reduction launch follows
    int epf = 0, epf_kernel = 0;         // epilogue prefetch: the mode the launch qualifies for / the mode of the kernel taken
    bool vec = false, stat_sums = false, pro_from_sums = false, bnr = false;      // vector loaders; the kernel adds its statistics to column sums / can build its prologue table from column sums / carries the BatchNorm-backward reduction
    bool stream_unfit = false;           // kFwd: a streaming-1x1 shape whose bias / prologue that kernel does not take
    bool row3 = false;                   // kX3: the row-shared main loop (x3_row3_matches)
};

// the split GEMMs whose three taps of a filter row share one staged A tile: forward and non-strided data gradient of a 3x3 / stride 1 /
// pad 1 conv (input and output maps coincide, a tap is a shift of the flat pixel index), K-steps that do not straddle taps
// DPFT_X3_ROW3=0|1 (A/B switch, default 1: on; read live, once per plan, like DPFT_FORCE_TILE -- tests run both forms in one process)
inline bool x3_row3_on() { const char* e = getenv("DPFT_X3_ROW3"); return !e || atoi(e) != 0; }
inline bool x3_row3_matches(const dpft_conv_desc* d, int gemm_c) {
    return x3_row3_on() && d->kh == 3 && d->kw == 3 && d->stride == 1 && d->pad == 1 && gemm_c % 32 == 0;
}
inline bool x3_tile(int bm, int bn) { return (bm == 128 && (bn == 128 || bn == 64)) || (bm == 64 && bn == 64); }

inline IgemmPlan plan_igemm(const dpft_conv_desc* d, IgemmKind kind, const IgemmIn& in, const PlanMode& mode) {
    const ConvTuning& tn = tuning();
    const ForceTile force = ForceTile();
    const bool dgrad = kind >= kDgrad, act16 = d->act16 != 0;
    GemmDims g = gemm_dims(d, dgrad);
    if (kind == kDgradClass) { g.M = in.M; g.ksteps = in.ksteps; }
    IgemmPlan p;
    // ---- kernels outside the implicit GEMM ----
    int stream_rows = 0;
    if (!dgrad && mode.compute != 1 && stream1x1_match(d, &stream_rows)) {
        // short reduction, wide output, large map: the streaming kernel, which has no bias and only the BatchNorm + ReLU prologue
        if (kind == kFwdBnact || (!in.bias && (!in.pro || in.pro_relu))) {
            p.kernel = kStream1x1; p.family = kFamF32; p.bm = stream_rows;
            p.stat_sums = in.sums && g.M < (1 << 22); p.pro_from_sums = true;
            return p;
        }
        p.stream_unfit = true;
    }
    if ((kind == kFwd && !in.pro && !in.stats) || kind == kDgrad) {
        if (conv16_matches(d)) { p.kernel = kConv16; return p; }
        const bool thin = kind == kFwd ? tn.thin_fwd && conv1x1_to16_matches(d)
                                       : d->C <= 4 && d->K % 4 == 0 && (size_t)d->C * d->kh * d->kw * d->K * 4 <= 40960;
        if (thin) { p.kernel = kThin; return p; }
    }
    // Parity classes pay when each class fills the chip on its own (4x fewer MFMAs); on small maps (radar encoders) the
    // stride^2 classes are stride^2 dependent launches of a few workgroups with the whole tap x channel loop inside
    // (170 us for a 4x16x7 map) -- there one split-K launch over all taps is ~6x faster despite the wasted taps.
    if (kind == kDgrad && d->stride > 1 && (g.C % BKV) == 0) {
        const int64_t class_wgs = (int64_t)cdiv((int64_t)d->B * cdiv(d->H, d->stride) * cdiv(d->W, d->stride), 64) * cdiv(g.N, 64);
        if (class_wgs >= kNumCU / 2 || !in.ws || act16) { p.kernel = kClasses; return p; }
    }
    // ---- tile and K split ----
    int taps = act16 ? 1 : taps_of(d);
    if ((kind == kFwd && in.pro && !in.pro_relu) || (kind == kDgrad && d->stride > 1) || kind == kDgradClass) taps = 1;
    const bool allow_big16 = kind == kFwd ? !in.pro && !in.bias : (kind == kDgrad || kind == kDgradRes);
    const int fix_kind = kind == kDgrad ? 2 : (kind == kDgradRes ? 4 : 1);
    TileChoice t = choose_tile(g.M, g.N, g.C, g.ksteps, taps, mode, force);
    const bool big16 = allow_big16 && big16_tile(d, g, dgrad, in.ws, force, t);
    // bf16 tensors split only with the in-launch fix-up (the reduction kernels write fp32 tensors), which the 256-row tiles alone have
    if ((act16 && !big16) || (big16 && !sk_fixup_ok(g, t.splits, fix_kind)) || kind == kDgradClass) t.splits = 1;
    p.fixup = sk_fixup_ok(g, t.splits, fix_kind);
    bool planes = in.planes && !act16 && !in.pro;
    if (kind == kFwdBnact) {
        // a K split (the latency-sized problems: batch-1 inference, the radar encoders' maps; the split kernels): the last
        // workgroup of a tile runs the whole inference epilogue (in-launch fix-up) -- no reduction launch, no elementwise pass
        p.fixup = p.fixup && in.ws && (t.x3 || (tn.bnact_fixup && t.vec && !conv16_matches(d)));
        if (!p.fixup && (!t.vec || t.splits > 1 || conv16_matches(d))) { p.kernel = kTwoPass; return p; }
        if (p.fixup) planes = false;
        // unsplit fp32 launch with a residual: the residual is read during the main loop instead of after it
        if ((tn.epf & 4) && !p.fixup && in.residual && !act16 && !planes && !t.x3 && (int64_t)g.M * g.N < (1ll << 29) && d->stride == 1 &&
            mode.compute != 1)
            p.epf = 3;
    }
    p.bnr = in.bnr && (t.splits == 1 || p.fixup);      // (with the fix-up the last split workgroup of a tile runs the unsplit epilogue)
    const bool epf_ok = t.splits == 1 && p.bnr && t.vec && (int64_t)g.M * g.N < (1ll << 29);
    // unsplit stride-1 data gradient that carries the reduction and nothing else in its epilogue: the reduction's operand (and
    // mask byte) is requested with the first tile (EpiPrefetch mode 2)
    if (kind == kDgrad && (tn.epf & 2) && epf_ok && !in.accumulate && d->stride == 1) p.epf = 2;
    // the full residual form (identity gradient + next BatchNorm's reduction, both ReLU masks as bytes), unsplit, with enough rows
    // to fill the chip with 128 x 64 tiles: its epilogue operands are fetched during the main loop (EpiPrefetch mode 1)
    if (kind == kDgradRes && (tn.epf & 1) && epf_ok && in.bnr_mask8 && in.res_mask8 && (int64_t)cdiv(g.M, 128) * cdiv(g.N, 64) >= kNumCU &&
        !force.set && !big16) {
        p.epf = 1;
        t.bm = 128; t.bn = 64;
    }
    if (t.splits > 1 && !p.fixup)
        p.reduce = kind == kDgradRes ? kReduceResidual
                   : (kind == kFwd && in.stats && !in.bias && (g.N % 64) == 0 && t.bm <= 128) ? kReduceStats : kReducePlain;
    // (the accumulators' low words hold 65 536 addends: tiles of >= 64 rows)
    p.stat_sums = kind == kFwd && in.sums && !in.bias && t.vec && (g.N & 3) == 0 && (t.splits == 1 || p.fixup) && g.M < (1 << 22);
    // ---- the kernel; what runs is a 64 x 64 tile for the all-tap strided data gradient, and for a forced 64 x 128 tile outside the
    // pipelined fp32 kernel (the only one that has it): the grid is counted in the tile that runs ----
    const bool pro = in.pro && !dgrad, x16 = act16, w16 = d->act16 == 2 && kind != kFwdBnact;      // (the inference epilogue takes fp32 weights)
    const bool nonlin = dgrad && t.vec && d->stride > 1 && kind != kDgradClass;
    // fp32, linear taps: the software-pipelined kernel (conv_pipe.h) -- LDS-DMA operands, one barrier per K-step
    const bool pipe = t.vec && mode.compute != 1 && (tn.pipe & 1) && !x16 && (!pro || in.pro_relu);
    const bool only64 = t.bm == 64 && t.bn == 128 && !pipe;
    p.vec = t.vec; p.splits = t.splits;
    p.bm = nonlin ? 64 : t.bm;
    p.bn = (nonlin || only64) ? 64 : t.bn;
    const int64_t tiles = (int64_t)cdiv(g.M, p.bm) * cdiv(g.N, p.bn);
    const bool t12864 = t.bm == 128 && t.bn == 64, t6464 = t.bm == 64 && t.bn == 64;
    if (!t.vec) {
        p.kernel = kGeneric;
    } else if (nonlin) {
        p.kernel = kAllTap; p.family = kFamF32;      // (no bf16-operand variant: fp32 MFMA in every compute mode)
    } else if (w16 && x16 && !pro) {
        // bf16 activations AND bf16 weights (act16 = 2): both operands go to the matrix cores untouched
        p.family = kFamBf16;
        p.kernel = t.bm == 256 ? kB16w : kPipe16;
        if (p.kernel == kPipe16) {
            if (dgrad && ((p.epf == 1 && t12864) || (p.epf == 2 && (t12864 || t6464)))) p.epf_kernel = p.epf;
            p.pbk = (t.bm == 128 || g.C % 128 != 0) ? 64 : 128;
        }
    } else if (planes && !x16 && !w16 && x3_tile(t.bm, t.bn)) {
        p.kernel = kX3Planes; p.family = kFamX3;      // operands given as three bf16 planes: the copy-only split kernel
    } else if ((t.x3 || (mode.compute == 2 && (tn.x3_all || force.set))) && mode.compute != 1 && !x16 && !w16 && (!pro || in.pro_relu) &&
               x3_tile(t.bm, t.bn)) {
        p.kernel = kX3; p.family = kFamX3;      // fp32 results from the bf16 matrix cores: three-term split of both operands, six MFMAs
        p.row3 = kind != kDgradClass && x3_row3_matches(d, g.C);
    } else if (pipe) {
        p.kernel = kPipe; p.family = kFamF32;
        const bool short_k = tn.shortk > 0 && g.Ktot <= tn.shortk;
        if (!pro && dgrad && ((p.epf == 1 && t12864) || (p.epf == 2 && (t12864 || (t6464 && !short_k))))) p.epf_kernel = p.epf;
        if (!pro && !dgrad && p.epf == 3 && (t.bm == 128 || (t6464 && !short_k))) p.epf_kernel = 3;
        p.pbk = (t6464 && !short_k) ? 64 : 32;
    } else {
        // K-split form (512 threads per tile) where the grid leaves the chip latency-bound: fewer than 3 workgroups per CU and
        // a reduction deep enough to amortise the hand-over.  Measured (tools/ksplit_ab.sh): -8...-10 % on the data gradients
        // of the 64 x 64-tile problems (layer-3 3x3: 102 -> 93.5 us), nothing or a loss on the forward kernels (prologue,
        // statistics epilogue) and on the 128-row tiles (one workgroup per CU either way) -- waves of ONE workgroup march in
        // step between barriers, so they do not fill each other's stalls the way a second resident workgroup does.  (A two-wave
        // 64 x 32 tile -- twice the workgroups -- was 15-90 % slower on the same problems: tools/tile6432.sh, removed.)
        const bool ks2 = dgrad && p.bm == 64 && p.bn == 64 &&
                         (tn.ksplit >= 0 ? tn.ksplit != 0 : (tiles * t.splits < kNumCU * 3 && cdiv(g.ksteps, t.splits) >= 8));
        p.kernel = ks2 ? kVecKS2 : kVec;
        p.family = mode.compute == 1 ? kFamBf16 : kFamF32;
    }
    // the split kernels and the pipelined fp32 kernel build their prologue table from column sums
    p.pro_from_sums = (t.x3 || (tn.pipe & 1)) && (p.kernel == kX3 || p.kernel == kPipe) && pro && in.pro_relu && (int64_t)12 * d->C <= 16384;
    return p;
}

// One output-pixel parity class of a strided data gradient (see IgemmArgs::sub_*): false where no tap reaches the class
struct DgradClass { int oh, ow, r0, s0, nr, ns, M, ksteps; };
inline bool dgrad_class(const dpft_conv_desc* d, int ph, int pw, DgradClass& c) {
    const int sp = d->stride;
    c.r0 = (ph + d->pad) % sp; c.s0 = (pw + d->pad) % sp;
    if (c.r0 >= d->kh || c.s0 >= d->kw || ph >= d->H || pw >= d->W) return false;
    c.oh = (d->H - ph + sp - 1) / sp; c.ow = (d->W - pw + sp - 1) / sp;
    c.nr = (d->kh - c.r0 + sp - 1) / sp; c.ns = (d->kw - c.s0 + sp - 1) / sp;
    c.M = d->B * c.oh * c.ow;
    c.ksteps = c.nr * c.ns * (d->K / BKV);
    return true;
}

// ---- the weight gradient -------------------------------------------------------------------------------------------
enum WgradKernel { kWgConv16Tiled, kWgConv16, kWgStem7, kWgThin1x1, kWgPipe16, kWgX3, kWgPipe, kWgVec, kWgGeneric };
enum { kWgReduceNone, kWgReduceSlab, kWgReduceSlabBias, kWgReduceWide16, kWgReduceWide4, kWgReduceSerial };
struct WgradIn {
    bool ws = false, pro = false, pro_relu = false;
    bool bias = false;      // the bias gradient is wanted from the same pass where the kernel has dy at hand
};
struct WgradPlan {
    WgradKernel kernel = kWgGeneric;
    int family = kFamVector, reduce = kWgReduceNone;
    bool vec = false;
    int blocks = 0;                      // thin paths (and only they): workgroups = slabs
    int bmn = 64, bnc = 64, ktiles = 0, ctiles = 0, splits = 1;
    int pk = BK;                         // pixels per step the kernel counts psteps in
    int64_t tiles = 0;
};
// pixel-split partial slabs are bounded by 512 splits and 64 MiB (the workspace contract)
inline int wgrad_max_splits(int64_t wbytes) { return (int)std::max<int64_t>(1, std::min<int64_t>(512, (64ll << 20) / wbytes)); }

inline WgradPlan plan_wgrad(const dpft_conv_desc* d, const WgradIn& in, const PlanMode& mode) {
    const ConvTuning& tn = tuning();
    WgradPlan p;
    const int taps = d->kh * d->kw, J = taps * d->C, M = d->B * d->OH * d->OW;
    // ---- thin-channel fast paths (conv16_kernels.h): no prologue, slabs in the workspace ----
    if (!in.pro && in.ws) {
        const bool unit = d->kh == 1 && d->kw == 1 && d->stride == 1 && d->pad == 0;
        if (conv16_matches(d)) {
            p.kernel = tn.wgrad16_tiled ? kWgConv16Tiled : kWgConv16;
            p.blocks = tn.wgrad16_tiled ? conv16_wgrad_tiled_blocks(d) : conv16_wgrad_blocks(d);
            if (in.bias && tn.wgrad16_tiled) p.reduce = kWgReduceSlabBias;
        } else if (tn.wgrad_stem && wgrad_stem7_matches(d)) {
            p.kernel = kWgStem7;
            p.blocks = std::max(1, std::min(kNumCU * 2, d->B * cdiv(d->OH, STEM_OH) * cdiv(d->OW, STEM_OW)));      // (<= 512 slabs: the workspace bound of the pixel-split path)
        } else if (unit && ((d->K == 16 && (d->C == 3 || d->C == 6)) || (d->K == 3 && d->C == 6))) {
            p.kernel = kWgThin1x1;
            p.blocks = (int)std::max<long>(1, std::min<long>(kNumCU * 2, (long)d->B * d->H * d->W / 1024));
            if (in.bias && d->K == 16) p.reduce = kWgReduceSlabBias;      // bias gradient as a virtual input channel of ones
        }
        if (p.blocks && !p.reduce) p.reduce = kWgReduceSlab;
        if (p.blocks) return p;
    }
    // ---- tile ----
    p.vec = (d->C % 32 == 0) && (d->K % 4 == 0);
    int psteps = cdiv(M, p.vec ? BKP : BK);
    auto set_tile = [&](int b) {      // square tiles, 32 x 128 for K <= 32
        p.bmn = b; p.bnc = b == 32 ? 128 : b;
        p.ktiles = cdiv(d->K, p.bmn); p.ctiles = cdiv(d->C, p.bnc);
        p.tiles = (int64_t)p.ktiles * p.ctiles * taps;
    };
    if (!p.vec) {
        p.ktiles = cdiv(d->K, 64); p.ctiles = cdiv(J, 64);
        p.tiles = (int64_t)p.ktiles * p.ctiles;
    } else {      // 64 x 64 also when 128 x 128 would leave < 8 output tiles to split over
        set_tile(d->K <= 32 ? 32 : (d->K >= 128 && d->C >= 128 && (int64_t)cdiv(d->K, 128) * cdiv(d->C, 128) * taps >= 8) ? 128 : 64);
    }
    // Pixel-splits: the grid should be ONE full round of workgroups -- 256 for the 128x128 tile, 512 (two per CU) for
    // the smaller ones -- and never spill a few workgroups into another round (tools/wgrad_sweep.sh: 36 tiles x 15
    // splits = 540 workgroups ran 25 % slower than 36 x 14 = 504 or 36 x 7 = 252).
    const int round_wgs = (p.vec && p.bmn == 128) ? kNumCU : kNumCU * 2;
    int splits = (int)std::max<int64_t>(1, round_wgs / p.tiles);
    {   // when one round would stay badly filled (e.g. 144 tiles), fill two rounds instead
        const int s2 = (int)std::max<int64_t>(1, 2 * round_wgs / p.tiles);
        const double f1 = (double)p.tiles * splits / round_wgs, f2 = (double)p.tiles * s2 / (2.0 * round_wgs);
        if (f1 < 0.8 && f2 > f1 + 0.1) splits = s2;
    }
    const int max_splits = wgrad_max_splits((int64_t)d->K * J * 4);
    if (splits > max_splits) splits = max_splits;
    if (splits > 1 && psteps / splits < 4) {
        // Few pixels (radar encoders: 84 ... 1800): a workgroup would get under four pixel steps, so its fixed costs and
        // the partial slabs decide.  tools/wgrad_small_sweep.sh: the 64x64 tile with about one workgroup per CU wins
        // by 2-4x over fewer, fatter workgroups (448 pixels, 256->1024: 11.9 us vs 48.3 us unsplit 128x128 tiles).
        if (p.vec && p.bmn == 128) set_tile(64);
        splits = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(kNumCU / p.tiles, psteps), max_splits));
    }
    if (splits < 1) splits = 1;
    if (const char* f = getenv("DPFT_FORCE_WGRAD")) {      // tuning aid, read live: "tile,splits" (tile 128 | 64 for the vec kernel)
        int tb, sp;
        if (p.vec && sscanf(f, "%d,%d", &tb, &sp) == 2 && (tb == 128 || tb == 64)) {
            set_tile(tb);
            splits = std::max(1, std::min(sp, max_splits));
        }
    }
    if (!in.ws) splits = 1;
    p.splits = splits;
    // ---- kernel ----
    const bool sq = p.bmn == 128 || p.bmn == 64;      // (not the 32 x 128 tile of K <= 32)
    p.pk = p.vec ? BKP : BK;
    if (!p.vec) {
        p.kernel = kWgGeneric;
    } else if (d->act16 && !in.pro && tn.wgrad16_pipe && sq && (d->C % 8) == 0 && (d->K % 8) == 0) {
        // both operands bf16 in memory, no prologue: LDS-DMA + transpose reads + bf16 MFMA (wgrad_pipe16_kernel)
        p.kernel = kWgPipe16; p.family = kFamBf16;
        p.pk = p.bmn == 128 ? 64 : 128;
    } else if ((tn.pipe & 2) && mode.compute != 1 && !d->act16 && (!in.pro || in.pro_relu) && sq) {
        // software-pipelined form (conv_pipe.h); the big multi-tap ones on the split kernels (conv_x3.hip), like their forward / data gradient
        const bool x3 = p.bmn == 128 && tn.wgrad_x3 && mode.split_on && (taps > 1 || tn.wgrad_x3_1x1) && 2.0 * M * (double)d->K * J >= 2e9;
        p.kernel = x3 ? kWgX3 : kWgPipe;
        p.family = x3 ? kFamX3 : kFamF32;
        p.pk = p.bmn == 128 ? 32 : 64;
    } else {
        p.kernel = kWgVec;      // mixed-precision mode: bf16 operands on the square tiles
        p.family = mode.compute == 1 && sq ? kFamBf16 : kFamF32;
    }
    if (splits > 1) {
        const int64_t n = (int64_t)d->K * J;
        p.reduce = ((n & 3) == 0 && splits >= 16) ? (n / 4 <= (int64_t)kNumCU * 64 ? kWgReduceWide16 : kWgReduceWide4) : kWgReduceSerial;
    }
    return p;
}

}  // namespace dpft
