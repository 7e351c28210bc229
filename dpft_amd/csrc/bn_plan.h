// What a launch of a BatchNorm-family pass will be, decided once: pure host functions of the shape, the storage type, the flags the
// launch site can observe and the tuning switches.  bn.hip's entries launch what a plan names; dpft_bn_plan_query reads the same plans.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../include/dpft_hip.h"
#include "host_consts.h"

namespace dpft {

constexpr int PB_TH = 4, PB_TW = 8, PB_CQ = 8;      // tiled max-pool backward: windows owned per tile (rows, cols), channel quads

// Every DPFT_* switch of bn.hip's host code, parsed once on first use
struct BnTuning {
    static int env(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
    int fixc = env("DPFT_BN_FIXC", 2);                        // fixed-channel forms (see fixc_grid).  0: off (A/B switch); U: quads in flight (fp32: act 1..2, apply 1..3)
    bool wide16 = env("DPFT_BN_WIDE16", 1) != 0;              // A/B switch: 16-byte accesses on bf16 tensors
    bool fat = env("DPFT_BN_FAT", 1) != 0;                    // A/B switch: the fp32 grid sized for two quads per thread and trip (see plan_f32)
    bool pool_bwd_tiled = env("DPFT_POOL_BWD_TILED", 1) != 0; // A/B switch: LDS-tiled max-pool backward
    int ew_blocks_per_cu = env("DPFT_EW_BLOCKS_PER_CU", 8);   // tuning aid
    const char* skip = skip_families();                       // timing experiment (wrong results): bnact, bnfinalize, bnfinK1024 -- the family's cost on the critical path
    bool skip_apply = env("DPFT_BN_SKIP_APPLY", 0) != 0;      // timing experiment (wrong gradients): what the apply pass costs on the step's critical path = the step time without it
};
inline const BnTuning& bn_tuning() { static const BnTuning t; return t; }
inline bool bn_skip(const char* family) { return bn_tuning().skip && strstr(bn_tuning().skip, family); }

// the process's switches, or the caller's five in their place (dpft_bn_plan_query: every setting from one process)
inline BnTuning bn_tuning_with(const dpft_bn_switches* sw) {
    BnTuning t = bn_tuning();
    if (sw) {
        t.fixc = sw->fixc; t.wide16 = sw->wide16 != 0; t.fat = sw->fat != 0;
        t.pool_bwd_tiled = sw->pool_bwd_tiled != 0; t.ew_blocks_per_cu = sw->ew_blocks_per_cu;
    }
    return t;
}

inline int ew_blocks(int64_t work_items, const BnTuning& t = bn_tuning()) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((work_items + 255) / 256, (int64_t)kNumCU * t.ew_blocks_per_cu));
}

// THE fixed-channel grid rule: can the launch's grid stride (blocks x 256) be a multiple of `kq` channel groups (K / 4 quads, or
// K / 8 octets for the 16-byte bf16 forms), so that a thread keeps its channels over all its trips?  May lower `blocks` to make it so.
inline bool fixc_grid(int kq, int64_t items, int& blocks, const BnTuning& t) {
    if (t.fixc <= 0 || items < 4096 || items >= (1ll << 30) || kq <= 0) return false;
    if ((256 % kq) == 0) return true;
    if ((kq % 256) != 0) return false;
    const int f = kq / 256;      // kq = 512 ...: the block count itself must carry the remaining factor
    if (blocks < f) return false;
    blocks -= blocks % f;
    return true;
}

inline dpft_bn_plan bn_plan_of(int form, int64_t grid_x, int per_thread, int lds_bytes = 0) {
    dpft_bn_plan p{};
    p.form = form; p.grid_x = grid_x; p.grid_y = 1; p.per_thread = per_thread; p.lds_bytes = lds_bytes;
    return p;
}

// fp32 tensors: the fixed-channel form with U = min(fixc, umax) quads per thread and trip where `allowed` and the grid rule holds,
// else the generic kernel.  U quads per thread and trip: a grid of n4 / (256 U) workgroups (inside the step a CU that also holds a split
// weight-gradient workgroup has room for ONE wave of these kernels per SIMD: the pass runs as rounds of 256 workgroups, so fewer,
// fatter ones) -- sized for two, whatever U, unless DPFT_BN_FAT=0
inline dpft_bn_plan plan_f32(int64_t n4, int K4, bool allowed, int umax, const BnTuning& t) {
    int blocks = ew_blocks(t.fat && t.fixc >= 2 ? (n4 + 1) / 2 : n4, t);
    if (!allowed || !fixc_grid(K4, n4, blocks, t)) return bn_plan_of(DPFT_BN_FORM_GENERIC, ew_blocks(n4, t), 1);
    const int U = std::min(t.fixc, umax);
    return bn_plan_of(U >= 3 ? DPFT_BN_FORM_FIXC3 : U == 2 ? DPFT_BN_FORM_FIXC2 : DPFT_BN_FORM_FIXC1, blocks, U);
}

// bf16 tensors: 16-byte accesses (an octet per lane) where K and the tensors' alignment allow, fixed-channel where the grid rule
// holds; else the generic kernel, 8 bytes per lane.  Both make two accesses per thread and trip.
inline dpft_bn_plan plan_bf16(int64_t n4, int K, bool aligned16, const BnTuning& t) {
    if (!(t.wide16 && K % 8 == 0 && aligned16)) return bn_plan_of(DPFT_BN_FORM_GENERIC, ew_blocks(n4, t), 2);
    int blocks = ew_blocks(n4 / 2, t);
    const bool fx = fixc_grid(K / 8, n4 / 2, blocks, t);
    return bn_plan_of(fx ? DPFT_BN_FORM_WIDE16_FIXC : DPFT_BN_FORM_WIDE16, blocks, 2);
}

// act: out = [relu](bn(y) [+ bn_r(res) | + res]).  The fp32 fixed-channel kernels write no fp32 copy (out32).
inline dpft_bn_plan plan_bn_act(int64_t M, int K, bool act16, bool out32, bool aligned16, const BnTuning& t) {
    const int64_t n4 = M * K / 4;
    return act16 ? plan_bf16(n4, K, aligned16, t) : plan_f32(n4, K / 4, !out32, 2, t);
}

// act from column sums (fp32): fixed-channel or declined (the generic kernel reads BN blocks only: the caller finalizes first).
// K / 4 < 256: the parameters go through a table in dynamic LDS, 6 floats per channel.
inline dpft_bn_plan plan_bn_act_sums(int64_t M, int K, const BnTuning& t) {
    dpft_bn_plan p = plan_f32(M * K / 4, K / 4, true, 2, t);
    if (p.form == DPFT_BN_FORM_GENERIC) return bn_plan_of(DPFT_BN_FORM_SUMS_DECLINED, 0, 0);
    p.form = DPFT_BN_FORM_SUMS_TAKEN;
    p.lds_bytes = K / 4 < 256 ? 24 * K : 0;
    return p;
}

// backward apply (see bn_bwd_apply_fixc_kernel); fp32: U = 3 exists (DPFT_BN_FIXC=3, an experiment switch)
inline dpft_bn_plan plan_bn_apply(int64_t M, int K, bool act16, bool aligned16, const BnTuning& t) {
    const int64_t n4 = M * K / 4;
    return act16 ? plan_bf16(n4, K, aligned16, t) : plan_f32(n4, K / 4, true, 3, t);
}

// backward reduce.  Tuned on MI355X (tools/bn_bench.py): 128 B wide channel slabs (8 float4) => 32 row groups per block and only
// 64 accumulators per block; at most 64 blocks per slab keeps the fp32 atomics on one accumulator <= 64-deep
// (the first version -- every block covering all K channels, 512 blocks -- spent most of its time in atomics).
inline dpft_bn_plan plan_bn_reduce(int64_t M, int K, bool act16) {
    const int K4 = K / 4;
    dpft_bn_plan p = bn_plan_of(DPFT_BN_FORM_GENERIC, 0, act16 ? 8 : 4);      // (rows per thread and trip)
    p.slab = std::min(K4, 8);
    p.slabs = cdiv(K4, p.slab);
    p.groups = 256 / p.slab;
    const int want_blocks = std::min(64, std::max(1, (kNumCU * 4) / p.slabs));
    p.rows_per_block = std::max<int64_t>((int64_t)p.groups * 4, (M + want_blocks - 1) / want_blocks);
    p.grid_x = cdiv(M, p.rows_per_block);
    p.grid_y = p.slabs;
    return p;
}

// stem max-pool backward: LDS tiles of 2 PB_TH x 2 PB_TW pixels x PB_CQ channel quads on the 3 x 3 / stride 2 / pad 1 geometry
// (one workgroup each), else a gather per input pixel
inline dpft_bn_plan plan_bn_pool_bwd(int B, int H, int W, int K, int PH, int PW, const BnTuning& t) {
    const int K4 = K / 4;
    if (t.pool_bwd_tiled && K4 % PB_CQ == 0 && PH == (H - 1) / 2 + 1 && PW == (W - 1) / 2 + 1)
        return bn_plan_of(DPFT_BN_FORM_POOL_TILED, (int64_t)B * (K4 / PB_CQ) * cdiv(H, 2 * PB_TH) * cdiv(W, 2 * PB_TW), 1);
    return bn_plan_of(DPFT_BN_FORM_GENERIC, ew_blocks((int64_t)B * H * W * K4, t), 1);
}

}  // namespace dpft
