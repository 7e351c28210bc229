// NHWC fp32 convolution family for gfx950 as MFMA implicit GEMM (v_mfma_f32_32x32x2_f32).
//
//   forward :  Y[M = B*OH*OW][N = K]  = A[M][kh*kw*C] * W^T        A gathered from x on the fly
//   dgrad   :  dX[M = B*H*W][N = C]   = A'[M][kh*kw*K] * Wt^T      A' gathered from dy (stride via
//                                                                   divisibility test), Wt = [C][taps][K]
//   wgrad   :  dW[K][tap][C]          = sum_pixels dY[p][k] * A[p][tap][c]
//
// Replaces the cuDNN kernels behind torchvision's ResNet/FPN in the reference
// (src/dprt/models/backbones/resnet.py:47-55,80-107; src/dprt/models/necks/fpn.py:39-43).
//
// Tiling (64-lane waves, 4 waves / workgroup): workgroup tile BM x BN, wave tile (RB*32) x (CB*32)
// of 32x32 MFMA blocks, BK = 32 per K-step staged through LDS with a register prefetch of the next
// step.  The A/B fragments are read from LDS with ds_read_b128: lanes 0-31 take k0..k0+3 and lanes
// 32-63 take k0+4..k0+7 of their row, and MFMA j consumes register j of both operands, i.e. a
// fixed permutation of the K order that both operands share (fp32 sums are order-independent up to
// rounding).  Rows are padded to 36 floats so the 16-lane groups of ds_read_b128 hit 16 distinct
// 16-byte slots.  Workgroup ids are remapped so that consecutive tiles (same A rows) share an XCD L2.
//
// Fused prologue (PRO): the producer's BatchNorm-apply + ReLU is applied to the A operand while it
// is staged (padding stays exactly zero).  Fused epilogue: per-tile per-channel (mean, M2) of the
// raw conv output for train-mode BatchNorm (combined later with Chan's formula: deterministic, no
// atomics, no E[x^2]-E[x]^2 cancellation).
#include "conv_core.h"

namespace dpft {


// ---------------------------------------------------------------------------------------------
// vector path: C % 32 == 0 (every bottleneck conv); float4 global loads, b128 LDS fragments
// ---------------------------------------------------------------------------------------------
// LIN = false: data gradient of a strided conv over ALL taps in one launch (small maps, see dpft_conv2d_nhwc_dgrad_f32):
// the source pixel is (oh + pad - r) / stride where that divides, not linear in the tap -- only that instantiation
// carries the divisions.
// BF16 = true (mixed-precision mode, dpft_conv_set_compute): the operands are rounded to bf16 (RNE) when a tile is written
// to LDS and multiplied with v_mfma_f32_32x32x16_bf16 (fp32 accumulation); tensors in memory stay fp32.
// (The three-term split of fp32 operands that this kernel carried as an experiment through rounds 1-4 is conv_x3.hip now.)
// KS = 2: 512 threads per tile -- waves 4..7 mirror waves 0..3 on the ODD K-groups of every step and hand their
// accumulators over through LDS at the end.  Same tile, same loads, same MFMA count, twice the waves per SIMD: the mid / late
// layers launch < 2 workgroups per CU (456 tiles at layer 3) and run latency-bound -- two of these kernels side by side
// finish in 1.55-1.68x the time of one (tools/occupancy_probe.py).
template <int BM, int BN, int WGM, int WGN, bool DGRAD, bool PRO, bool LIN = true, bool BF16 = false, int KS = 1>
__global__ __launch_bounds__(64 * WGM * WGN * KS) void igemm_vec_kernel(IgemmArgs a) {
    static_assert(KS == 1 || KS == 2, "K-split form: two wave sets");
    constexpr int NT = 64 * WGM * WGN * KS, ROWS = NT / 16;      // loader: 16 lanes x 16 bytes per row, ROWS rows per pass
    constexpr int RB = BM / WGM / 32, CB = BN / WGN / 32;
    constexpr int AP = BM / ROWS, BP = BN / ROWS;      // ROWS rows x 16 chunks (of 16 B) per loader pass
    static_assert(WGM * WGN == 4 && RB >= 1 && CB >= 1, "bad tile");
    extern __shared__ __attribute__((aligned(16))) float smem[];   // (BM + BN) * LDK floats
    float* As = smem;
    float* Bs = smem + BM * LDK;
    // bf16 tiles: rows of 64 + 8 halfs (144 B: 16 consecutive rows start in 16 different 16-byte bank groups)
    __bf16* Ah = reinterpret_cast<__bf16*>(smem);
    __bf16* Bh = Ah + BM * LDKH;

    const int tid = threadIdx.x, lane = tid & 63, wave = (tid >> 6) & 3;
    const int kh = KS == 1 ? 0 : tid >> 8;            // which K-groups of a step this wave multiplies (4-wave tiles)
    const int wm = wave / WGN, wn = wave % WGN;
    int mt, nt, split;
    decode_tile(a, mt, nt, split);
    const int m0 = mt * BM, n0 = nt * BN;

    const int chunk = tid & 15, rowl = tid >> 4;
    // ---- operand addressing --------------------------------------------------------------------------------------
    // fp32 "MFMA" runs on the vector ALUs of gfx950 (its peak IS the vector fp32 peak; tools/probes/mfma_valu_overlap:
    // MFMA + VALU time add up, at any occupancy), so every address / mask / clamp instruction of the loader is paid in
    // matrix throughput.  The loader therefore costs no vector instruction per K-step:
    //  * raw buffer loads: the hardware range check returns 0 for an offset beyond the tensor (voffset + soffset are
    //    both checked on gfx950, dword by dword: tools/probes/buffer_range.hip), which serves the zero padding, rows
    //    >= M and weight rows >= N without clamps, selects or a zeroing pass;
    //  * one 32-bit byte offset per loader row, recomputed only when the filter tap changes (every C/64 steps), from
    //    per-row filter-row / filter-column validity bits built once; the channel offset of the step travels in the
    //    scalar soffset.
    const bool sub = DGRAD && a.sub_step > 1;
    constexpr bool lin = LIN;      // source pixel is linear in the tap: forward, stride-1 dgrad, parity-class dgrad
    const int roww = sub ? a.sub_ow : a.OW;
    const int ohw = sub ? a.sub_oh * a.sub_ow : a.OH * a.OW;
    const int ntap_s = sub ? a.sub_ns : a.kw;
    const int ntap_r = sub ? a.sub_nr : a.kh;      // kh, kw <= 8 (host side)
    constexpr unsigned OOB = 0x80000000u;
    int a_h0[AP], a_w0[AP], a_row[AP];      // tap-origin pixel (may lie outside the image) and its element offset
    unsigned a_mask[AP];                    // which filter rows / columns read a real pixel (see below)
#pragma unroll
    for (int i = 0; i < AP; ++i) {
        const int m = m0 + rowl + ROWS * i;
        const bool ok = m < a.M;
        const int mm = ok ? m : 0;
        const int b = mm / ohw;
        const int rem = mm - b * ohw;
        int oh = rem / roww, ow = rem - oh * roww;
        int h0, w0;
        if (!DGRAD) {
            h0 = oh * a.stride - a.pad;
            w0 = ow * a.stride - a.pad;
        } else if (sub) {      // (oh,ow) = sub-grid index; source row = index + q0 - tap index (see IgemmArgs::sub_*)
            h0 = oh + (a.sub_ph + a.pad - a.sub_r0) / a.sub_step;
            w0 = ow + (a.sub_pw + a.pad - a.sub_s0) / a.sub_step;
        } else {
            h0 = oh + a.pad;
            w0 = ow + a.pad;
        }
        a_h0[i] = h0; a_w0[i] = w0;
        a_row[i] = lin ? ((b * a.H + h0) * a.W + w0) * a.C : b * a.H * a.W * a.C;
        // tap validity is separable: bits 0..7 = filter rows that land inside the image, bits 8..15 = filter columns
        unsigned mask = 0;
        for (int ri = 0; ri < ntap_r; ++ri) {
            int hi;
            bool v = ok;
            if (!DGRAD) hi = h0 + ri;
            else if (lin) hi = h0 - ri;
            else {
                const int th = h0 - ri;
                hi = th / a.stride;
                v = v && th >= 0 && hi * a.stride == th;
            }
            mask |= (v && (unsigned)hi < (unsigned)a.H) ? (1u << ri) : 0u;
        }
        for (int si = 0; si < ntap_s; ++si) {
            int wi;
            bool v = ok;
            if (!DGRAD) wi = w0 + si;
            else if (lin) wi = w0 - si;
            else {
                const int tw = w0 - si;
                wi = tw / a.stride;
                v = v && tw >= 0 && wi * a.stride == tw;
            }
            mask |= (v && (unsigned)wi < (unsigned)a.W) ? (256u << si) : 0u;
        }
        a_mask[i] = mask;
    }
    unsigned b_off[BP];      // byte offset of weight row n (+ this lane's 16-byte chunk); OOB for rows >= N
#pragma unroll
    for (int i = 0; i < BP; ++i) {
        const int n = n0 + rowl + ROWS * i;
        b_off[i] = n < a.N ? (unsigned)(n * a.Ktot + chunk * 4) * 4u : OOB;
    }
    const __amdgpu_buffer_rsrc_t rsrc_a =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, a.B * a.H * a.W * a.C * (a.x16 ? 2 : 4), 0x00020000);
    const bool x16 = a.x16 != 0;
    const bool raw_a = BF16 && !PRO && x16;      // bf16 tensor -> bf16 LDS tile without arithmetic: copy the bits
    const __amdgpu_buffer_rsrc_t rsrc_b =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, a.N * a.Ktot * 4, 0x00020000);
    const int cpt = a.C / BKV;  // K-steps per filter tap
    unsigned a_off[AP];         // byte offsets of the current tap (OOB where the tap misses the image)
    unsigned a_valid_tap = 0;   // bit i: row i of the current tap is a real pixel
    int cur_tap = -1;
    auto set_tap = [&](int tap) {
        const int ri = tap / ntap_s, si = tap - ri * ntap_s;
        const int tapoff = (DGRAD ? -1 : 1) * (ri * a.W + si) * a.C;      // linear case
        unsigned valid = 0;
#pragma unroll
        for (int i = 0; i < AP; ++i) {
            const bool v = ((a_mask[i] >> ri) & (a_mask[i] >> (8 + si)) & 1u) != 0;
            int e;
            if (lin) {
                e = a_row[i] + tapoff;
            } else {
                const int hi = (a_h0[i] - ri) / a.stride, wi = (a_w0[i] - si) / a.stride;
                e = a_row[i] + (hi * a.W + wi) * a.C;
            }
            a_off[i] = v ? (unsigned)(e + chunk * 4) * 4u : OOB;
            valid |= v ? (1u << i) : 0u;
        }
        a_valid_tap = valid;
        cur_tap = tap;
    };

    // Raw operand registers of the next DEPTH K-steps (register ring).  Loads are issued two steps ahead:
    // under load HBM/L2 latency exceeds one step of MFMA work, and a wait right behind the MFMAs stalls every
    // wave of the workgroup at once (probe: +30 % at 64x64).  The producer's BN+ReLU (PRO) is applied when a
    // register set is written to LDS, never earlier: consuming a load puts its latency in front of the compute.
    constexpr int DEPTH = (BM * BN >= 128 * 128) ? 1 : 2;       // 128x128 would exceed the VGPR budget at depth 2
    f32x4 ra[DEPTH][AP], rbv[DEPTH][BP], p_mu[DEPTH], p_sc[DEPTH], p_sh[DEPTH];
    unsigned a_valid[DEPTH];
    // data-gradient kernels: load_tile is called once per K-step in step order, so (tap, channel offset, weight offset)
    // are running scalars instead of kt / cpt and two more divisions per step (-8 % on the 3x3 256-channel dgrad; the
    // forward kernels measured 2-7 % SLOWER with the same change and keep the plain form)
    int run_tap = -1, run_c0 = 0, run_koff = 0;
    auto load_tile = [&](auto S, int kt) {
        constexpr int sidx = decltype(S)::value;
        int c0, koff;
        if constexpr (DGRAD) {
            if (run_tap < 0) {      // first call of this workgroup
                run_tap = kt / cpt;
                run_c0 = (kt - run_tap * cpt) * BKV;
            }
            if (run_tap != cur_tap) {
                set_tap(run_tap);
                const int ri = run_tap / ntap_s, si = run_tap - ri * ntap_s;
                run_koff = (sub ? (a.sub_r0 + a.sub_step * ri) * a.kw + a.sub_s0 + a.sub_step * si : run_tap) * a.C;
            }
            c0 = run_c0;
            koff = run_koff + c0;
            run_c0 += BKV;
            if (run_c0 == a.C) { run_c0 = 0; ++run_tap; }
        } else {
            const int tap = kt / cpt;
            c0 = (kt - tap * cpt) * BKV;
            if (tap != cur_tap) set_tap(tap);      // uniform
            const int r = tap / a.kw, s_ = tap - r * a.kw;
            koff = (r * a.kw + s_) * a.C + c0;      // == kt * BKV
        }
        if (PRO) {
            p_mu[sidx] = *reinterpret_cast<const f32x4*>(a.pro + c0 + chunk * 4);
            p_sc[sidx] = *reinterpret_cast<const f32x4*>(a.pro + a.C + c0 + chunk * 4);
            p_sh[sidx] = *reinterpret_cast<const f32x4*>(a.pro + 2 * a.C + c0 + chunk * 4);
            // bf16 operands: one fma per element, bn(v) = v * scale + (beta - mean * scale).  (The fp32 path subtracts the
            // mean first: that form keeps digits when |mean| >> sigma; with an 8-bit mantissa downstream it buys nothing.)
            if (BF16) p_sh[sidx] -= p_mu[sidx] * p_sc[sidx];
        }
        // one uniform branch around the whole batch of loads (a select per load would put every load in its own basic
        // block and serialise them).  bf16 tensors arrive as raw bits (lanes 0,1 of the quad) and are widened only when
        // the register set is consumed in store_tile: touching a load here would put its latency in front of the MFMAs.
        if (x16) {
#pragma unroll
            for (int i = 0; i < AP; ++i) ld4_raw16(ra[sidx][i], rsrc_a, a_off[i], c0 * 4);
        } else {
#pragma unroll
            for (int i = 0; i < AP; ++i) ra[sidx][i] = ld4(rsrc_a, a_off[i], c0 * 4, false);
        }
        a_valid[sidx] = a_valid_tap;
#pragma unroll
        for (int i = 0; i < BP; ++i)
            rbv[sidx][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_b, (int)b_off[i], koff * 4, 0));
    };
    auto store_bf16 = [&](__bf16* dst, f32x4 v) {      // rounded to bf16 (RNE)
        *reinterpret_cast<bf16x4*>(dst) = __builtin_convertvector(v, bf16x4);
    };
    const bool pro_mask = a.kh * a.kw > 1 || a.pad > 0;      // padding exists: BN(0) != 0 must be forced back to 0
    auto store_tile = [&](auto S) {
        constexpr int sidx = decltype(S)::value;
        // (storage-format branches stay OUTSIDE the unrolled loops: a branch per register quad puts every store in its
        // own basic block with its own wait)
        if (BF16 && raw_a) {
#pragma unroll
            for (int i = 0; i < AP; ++i)
                *reinterpret_cast<u32x2*>(&Ah[(rowl + ROWS * i) * LDKH + chunk * 4]) =
                    u32x2{__float_as_uint(ra[sidx][i][0]), __float_as_uint(ra[sidx][i][1])};
        } else {
            if (x16) {
#pragma unroll
                for (int i = 0; i < AP; ++i)
                    ra[sidx][i] = widen_bf16x4(u32x2{__float_as_uint(ra[sidx][i][0]), __float_as_uint(ra[sidx][i][1])});
            }
#pragma unroll
            for (int i = 0; i < AP; ++i) {
                f32x4 val = ra[sidx][i];
                if (PRO) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float t = BF16 ? fmaf(val[e], p_sc[sidx][e], p_sh[sidx][e])
                                       : fmaf(val[e] - p_mu[sidx][e], p_sc[sidx][e], p_sh[sidx][e]);
                        val[e] = a.pro_relu ? fmaxf(t, 0.f) : t;
                    }
                    if (pro_mask && !((a_valid[sidx] >> i) & 1u)) val = f32x4{0.f, 0.f, 0.f, 0.f};
                }
                if (BF16) store_bf16(&Ah[(rowl + ROWS * i) * LDKH + chunk * 4], val);
                else *reinterpret_cast<f32x4*>(&As[(rowl + ROWS * i) * LDK + chunk * 4]) = val;
            }
        }
#pragma unroll
        for (int i = 0; i < BP; ++i) {
            if (BF16) store_bf16(&Bh[(rowl + ROWS * i) * LDKH + chunk * 4], rbv[sidx][i]);
            else *reinterpret_cast<f32x4*>(&Bs[(rowl + ROWS * i) * LDK + chunk * 4]) = rbv[sidx][i];
        }
    };

    // NACC > 1 = K-interleaved partial accumulators per 32x32 block (summed in the epilogue) to break the
    // single-accumulator MFMA chain of the small wave tiles (PMC at 64x64: MFMA busy 44 %, SQ_WAIT_INST_ANY
    // 62 %).  Measured: no gain at 64x64 (70 vs 69 TF) and -15 % at 128x64 (occupancy), so it stays off.
    constexpr int NACC = 1;
    f32x16 accp[NACC][RB][CB];
#pragma unroll
    for (int q = 0; q < NACC; ++q)
#pragma unroll
        for (int i = 0; i < RB; ++i)
#pragma unroll
            for (int j = 0; j < CB; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) accp[q][i][j][r] = 0.f;

    const int kt_begin = split * a.ksteps_per_split;
    const int kt_end = min(a.ksteps, kt_begin + a.ksteps_per_split);
    const float* a_frag = As + (wm * RB * 32 + (lane & 31)) * LDK + (lane >> 5) * 4;
    const float* b_frag = Bs + (wn * CB * 32 + (lane & 31)) * LDK + (lane >> 5) * 4;
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, DEPTH - 1>;      // == S0 when DEPTH == 1

    // The fragments of K-group kg+1 are read from LDS BEFORE the MFMAs of group kg are issued (two register sets;
    // sched_barrier keeps the order -- left alone the scheduler reads a group right before its use, and the wave then
    // waits out the LDS latency with nothing in the pipe).
    const __bf16* a_fragh = Ah + (wm * RB * 32 + (lane & 31)) * LDKH + (lane >> 5) * 8;
    const __bf16* b_fragh = Bh + (wn * CB * 32 + (lane & 31)) * LDKH + (lane >> 5) * 8;
    auto compute_bf16 = [&]() {      // 4 K-groups of 16: lane l holds k = 8 * (l / 32) .. + 7 of row / column l % 32
        bf16x8 af[2][RB], bf[2][CB];
        auto frags = [&](int set, int kg) {
#pragma unroll
            for (int i = 0; i < RB; ++i) af[set][i] = *reinterpret_cast<const bf16x8*>(a_fragh + i * 32 * LDKH + kg * 16);
#pragma unroll
            for (int j = 0; j < CB; ++j) bf[set][j] = *reinterpret_cast<const bf16x8*>(b_fragh + j * 32 * LDKH + kg * 16);
        };
        constexpr int NG = BKV / 16 / KS;      // K-groups of this wave: kg = KS * g + kh
        frags(0, kh);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g + 1 < NG) frags((g + 1) & 1, KS * (g + 1) + kh);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int j = 0; j < CB; ++j)
                    accp[0][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[g & 1][i], bf[g & 1][j], accp[0][i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto compute_f32 = [&]() {
        f32x4 af[2][RB], bf[2][CB];
        auto frags = [&](int set, int kg) {
#pragma unroll
            for (int i = 0; i < RB; ++i)
                af[set][i] = *reinterpret_cast<const f32x4*>(a_frag + i * 32 * LDK + kg * 8);
#pragma unroll
            for (int j = 0; j < CB; ++j)
                bf[set][j] = *reinterpret_cast<const f32x4*>(b_frag + j * 32 * LDK + kg * 8);
        };
        constexpr int NG = BKV / 8 / KS;      // K-groups of this wave: kg = KS * g + kh
        frags(0, kh);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g + 1 < NG) frags((g + 1) & 1, KS * (g + 1) + kh);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < RB; ++i)
#pragma unroll
                    for (int j = 0; j < CB; ++j)
                        accp[e % NACC][i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[g & 1][i][e], bf[g & 1][j][e],
                                                                                    accp[e % NACC][i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    auto compute = [&]() {
        if constexpr (BF16) compute_bf16();
        else compute_f32();
    };

    // tile t (relative to kt_begin) lives in register set t % DEPTH
    const bool ab_ld = !(a.ablate & 1), ab_st = !(a.ablate & 2), ab_mm = !(a.ablate & 8);
    if (kt_begin < kt_end) load_tile(S0{}, kt_begin);
    if (DEPTH == 2 && kt_begin + 1 < kt_end) load_tile(S1{}, kt_begin + 1);
    if (kt_begin < kt_end) {
        store_tile(S0{});
        if (kt_begin + DEPTH < kt_end) load_tile(S0{}, kt_begin + DEPTH);
    }
    __syncthreads();
    for (int kt = kt_begin; kt < kt_end; kt += DEPTH) {
        // ---- step kt: the next tile (kt+1) is in set 1 % DEPTH ----
        if (ab_mm) compute();
        __syncthreads();
        if (kt + 1 < kt_end) {
            if (ab_st) store_tile(S1{});
            if (kt + 1 + DEPTH < kt_end && ab_ld) load_tile(S1{}, kt + 1 + DEPTH);
        }
        __syncthreads();
        if (DEPTH == 2) {
            if (kt + 1 >= kt_end) break;
            // ---- step kt+1: the next tile (kt+2) is in set 0 ----
            if (ab_mm) compute();
            __syncthreads();
            if (kt + 2 < kt_end) {
                if (ab_st) store_tile(S0{});
                if (kt + 2 + DEPTH < kt_end && ab_ld) load_tile(S0{}, kt + 2 + DEPTH);
            }
            __syncthreads();
        }
    }
    f32x16 (&acc)[RB][CB] = accp[0];
    if (NACC == 2) {
#pragma unroll
        for (int i = 0; i < RB; ++i)
#pragma unroll
            for (int j = 0; j < CB; ++j) acc[i][j] += accp[NACC - 1][i][j];
    }
    if constexpr (KS == 2) {      // waves 4..7 hand their partial sums to waves 0..3: [wave][block][register][lane] in LDS
        static_assert((size_t)4 * RB * CB * 16 * 64 <= (size_t)(BM + BN) * LDK, "hand-over buffer exceeds the operand tiles");
        __syncthreads();          // the operand tiles are dead
        float* hand = smem + ((size_t)wave * RB * CB * 16) * 64 + lane;
        if (kh == 1) {
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int j = 0; j < CB; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) hand[((i * CB + j) * 16 + r) * 64] = acc[i][j][r];
        }
        __syncthreads();
        if (kh == 0) {
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int j = 0; j < CB; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] += hand[((i * CB + j) * 16 + r) * 64];
        }
    }
    if (a.ablate & 4) {      // keep the accumulators live without the epilogue
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < RB; ++i)
#pragma unroll
            for (int j = 0; j < CB; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) t += acc[i][j][r];
        if (t == 1.2345e-30f) a.y[0] = t;
        return;
    }
    igemm_epilogue<BM, BN, WGM, WGN, RB, CB, NT>(a, acc, m0, n0, mt, split, smem);
}

// ---------------------------------------------------------------------------------------------
// generic path: any C (stem C=3, FPN C=3/6/16); K flattened as (tap, c); scalar gathers
// workgroup tile 128 x BN (BN = 32 or 64), waves 4 x 1
// ---------------------------------------------------------------------------------------------
template <int BN, bool DGRAD>
__global__ __launch_bounds__(256) void igemm_gen_kernel(IgemmArgs a) {
    constexpr int BM = 128, WGM = 4, WGN = 1, RB = 1, CB = BN / 32;
    constexpr int KPB = BN / 8;  // k elements per thread for the B tile
    constexpr int SMEM = ((BM + BN) * LDG > BM * (BN + 4)) ? (BM + BN) * LDG : BM * (BN + 4);
    __shared__ __attribute__((aligned(16))) float smem[SMEM];
    float* As = smem;
    float* Bs = smem + BM * LDG;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave;
    int mt, nt, split;
    decode_tile(a, mt, nt, split);
    const int m0 = mt * BM, n0 = nt * BN;

    // A: one row per thread, 16 consecutive k
    const int arow = tid & 127, akh = tid >> 7;
    int bh, bw;
    const float* abase;
    {
        const int m = m0 + arow;
        const bool ok = m < a.M;
        const int mm = ok ? m : 0;
        const int ohw = a.OH * a.OW;
        const int b = mm / ohw;
        const int rem = mm - b * ohw;
        const int oh = rem / a.OW, ow = rem - oh * a.OW;
        if (!DGRAD) {
            bh = ok ? oh * a.stride - a.pad : -(1 << 28);
            bw = ow * a.stride - a.pad;
        } else {
            bh = ok ? oh + a.pad : -(1 << 28);
            bw = ow + a.pad;
        }
        abase = a.x + (size_t)b * a.H * a.W * a.C;
    }
    const int brow = tid % BN, bkq = tid / BN;
    const bool bok = (n0 + brow) < a.N;
    const float* bbase = a.w + (size_t)(bok ? n0 + brow : 0) * a.Ktot;

    float ra[16], rbv[KPB];
    auto load_tile = [&](int kt) {
        int k = kt * BK + akh * 16;
        int tap = k / a.C;
        int c = k - tap * a.C;
        int r = tap / a.kw, s = tap - r * a.kw;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            int hi, wi;
            bool v = (k + e) < a.Ktot;
            if (!DGRAD) {
                hi = bh + r;
                wi = bw + s;
                v = v && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
            } else {
                const int th = bh - r, tw = bw - s;
                v = v && th >= 0 && tw >= 0;
                hi = th / a.stride;
                wi = tw / a.stride;
                v = v && (hi * a.stride == th) && (wi * a.stride == tw) && hi < a.H && wi < a.W;
            }
            ra[e] = v ? abase[((size_t)hi * a.W + wi) * a.C + c] : 0.f;
            if (++c == a.C) {
                c = 0;
                if (++s == a.kw) {
                    s = 0;
                    ++r;
                }
            }
        }
        const int kb = kt * BK + bkq * KPB;
#pragma unroll
        for (int e = 0; e < KPB; ++e) rbv[e] = (bok && (kb + e) < a.Ktot) ? bbase[kb + e] : 0.f;
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int e = 0; e < 16; ++e) As[arow * LDG + akh * 16 + e] = ra[e];
#pragma unroll
        for (int e = 0; e < KPB; ++e) Bs[brow * LDG + bkq * KPB + e] = rbv[e];
    };

    f32x16 acc[RB][CB];
#pragma unroll
    for (int j = 0; j < CB; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][j][r] = 0.f;

    const int kt_begin = split * a.ksteps_per_split;
    const int kt_end = min(a.ksteps, kt_begin + a.ksteps_per_split);
    const float* a_frag = As + (wm * 32 + (lane & 31)) * LDG + (lane >> 5);
    const float* b_frag = Bs + (lane & 31) * LDG + (lane >> 5);
    if (kt_begin < kt_end) {
        load_tile(kt_begin);
        store_tile();
    }
    __syncthreads();
    for (int kt = kt_begin; kt < kt_end; ++kt) {
        const bool more = kt + 1 < kt_end;
        if (more) load_tile(kt + 1);
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            const float av = a_frag[kk * 2];
#pragma unroll
            for (int j = 0; j < CB; ++j)
                acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b_frag[j * 32 * LDG + kk * 2],
                                                                 acc[0][j], 0, 0, 0);
        }
        __syncthreads();
        if (more) store_tile();
        __syncthreads();
    }
    igemm_epilogue<BM, BN, WGM, WGN, RB, CB>(a, acc, m0, n0, mt, split, smem);
}

// split-K reduce: y = sum_s partial[s] (+bias)
__global__ void splitk_reduce_kernel(const float* __restrict__ partial, const float* __restrict__ bias,
                                     float* __restrict__ y, int64_t MN, int N, int splits, int accumulate) {
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= MN) return;
    if (i + 3 < MN && (N % 4) == 0) {
        f32x4 s = *reinterpret_cast<const f32x4*>(partial + i);
        for (int k = 1; k < splits; ++k) {
            f32x4 t = *reinterpret_cast<const f32x4*>(partial + (size_t)k * MN + i);
            s += t;
        }
        if (bias) {
            const int c = (int)(i % N);
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] += bias[c + e];
        }
        if (accumulate) s += *reinterpret_cast<const f32x4*>(y + i);
        *reinterpret_cast<f32x4*>(y + i) = s;
    } else {
        for (int e = 0; e < 4 && i + e < MN; ++e) {
            float s = 0.f;
            for (int k = 0; k < splits; ++k) s += partial[(size_t)k * MN + i + e];
            if (bias) s += bias[(i + e) % N];
            if (accumulate) s += y[i + e];
            y[i + e] = s;
        }
    }
}

// split-K reduce of a forward conv WITH the BatchNorm tile statistics of the reduced output (what the non-split kernel's
// epilogue produces): one launch instead of reduce + bn_stats on the radar encoders' small maps, where every dependent
// launch costs more than the work in it.  block = one statistics tile (tile_rows <= 128 rows) x 64 columns;
// thread = one float4 column chunk x every 16th row.  N % 64 == 0.
__global__ __launch_bounds__(256) void splitk_reduce_stats_kernel(const float* __restrict__ partial, float* __restrict__ y,
                                                                  float* __restrict__ stats, int64_t M, int N, int splits,
                                                                  int tile_rows) {
    __shared__ f32x4 red[16][16];
    __shared__ f32x4 smean[16];
    const int cl = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int tile = blockIdx.x, c = blockIdx.y * 64 + cl * 4;
    const int64_t r0 = (int64_t)tile * tile_rows, MN = M * N;
    const int cnt = (int)min((int64_t)tile_rows, M - r0);
    f32x4 v[8];
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int r = rg + i * 16;
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (r < cnt) {
            const int64_t o = (r0 + r) * N + c;
            f32x4 a = *reinterpret_cast<const f32x4*>(partial + o);
            for (int k = 1; k < splits; ++k) a += *reinterpret_cast<const f32x4*>(partial + (size_t)k * MN + o);
            *reinterpret_cast<f32x4*>(y + o) = a;
            v[i] = a;
            sum += a;
        }
    }
    red[rg][cl] = sum;
    __syncthreads();
    if (rg == 0) {
        f32x4 t = red[0][cl];
        for (int i = 1; i < 16; ++i) t += red[i][cl];
        smean[cl] = t * (1.0f / (float)cnt);
    }
    __syncthreads();
    const f32x4 mean = smean[cl];
    f32x4 m2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (rg + i * 16 < cnt) {
            const f32x4 dlt = v[i] - mean;
            m2 += dlt * dlt;
        }
    __syncthreads();
    red[rg][cl] = m2;
    __syncthreads();
    if (rg == 0) {
        f32x4 t = red[0][cl];
        for (int i = 1; i < 16; ++i) t += red[i][cl];
        *reinterpret_cast<f32x4*>(stats + ((size_t)tile * 2 + 0) * N + c) = mean;
        *reinterpret_cast<f32x4*>(stats + ((size_t)tile * 2 + 1) * N + c) = t;
    }
}

// weight-gradient slabs: many splits (up to 512) of a result that can be as small as 64 x 64 -- the slab index is
// spread over PARTS lanes per output chunk (the serial walk above needs `splits` dependent trips per thread)
template <int PARTS>
__global__ __launch_bounds__(256) void splitk_reduce_wide_kernel(const float* __restrict__ partial, float* __restrict__ y,
                                                                 int64_t MN, int splits) {
    constexpr int CH = 256 / PARTS;      // float4 chunks per block
    __shared__ f32x4 red[256];
    const int ch = threadIdx.x % CH, part = threadIdx.x / CH;
    const int64_t i = ((int64_t)blockIdx.x * CH + ch) * 4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (i < MN)
        for (int k = part; k < splits; k += PARTS) s += *reinterpret_cast<const f32x4*>(partial + (size_t)k * MN + i);
    red[threadIdx.x] = s;
    __syncthreads();
    if (part == 0 && i < MN) {
#pragma unroll
        for (int q = 1; q < PARTS; ++q) s += red[q * CH + ch];
        *reinterpret_cast<f32x4*>(y + i) = s;
    }
}

// split-K reduce with the masked residual: y = sum_s partial[s] + (mask > 0 ? src : 0)
__global__ void splitk_reduce_residual_kernel(const float* __restrict__ partial, const float* __restrict__ src,
                                              const float* __restrict__ mask, float* __restrict__ y, int64_t MN,
                                              int splits) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= MN) return;
    float s = 0.f;
    for (int k = 0; k < splits; ++k) s += partial[(size_t)k * MN + i];
    y[i] = s + (mask[i] > 0.f ? src[i] : 0.f);
}

// ---------------------------------------------------------------------------------------------
// wgrad: dW[n][tap][c] = sum_p dY[p][n] * act(x)[p@tap][c]
// LDS holds [32 pixels][BMn] of dY and [32 pixels][BNc] of x; both fragments are ds_read_b32
// (consecutive lanes -> consecutive channels, conflict free).
// ---------------------------------------------------------------------------------------------

// BF16 = true (mixed-precision mode, square tiles): both operands are rounded to bf16 and TRANSPOSED on their
// way into LDS ([channel][pixel], so that a lane finds the 8 consecutive reduction indices v_mfma_f32_32x32x16_bf16
// wants); see store_tile.
template <int BMn, int BNc, int WGM, int WGN, bool PRO, bool BF16 = false>
__global__ __launch_bounds__(256) void wgrad_vec_kernel(WgradArgs a) {
    static_assert(!BF16 || (BMn == BNc && (BMn == 128 || BMn == 64)), "bf16 weight gradient: 128 x 128 and 64 x 64 tiles");
    constexpr int RB = BMn / WGM / 32, CB = BNc / WGN / 32;
    constexpr int YCH = BMn / 4, XCH = BNc / 4;        // float4 chunks per pixel row
    constexpr int YRP = 256 / YCH, XRP = 256 / XCH;    // pixel rows per pass
    constexpr int YP = BKP / YRP, XP = BKP / XRP;
    static_assert(WGM * WGN == 4 && YP >= 1 && XP >= 1, "bad wgrad tile");
    constexpr int SMEM_FLOATS = BKP * (BMn + BNc);
    __shared__ __attribute__((aligned(16))) float smem[SMEM_FLOATS];
    float* Ys = smem;
    float* Xs = smem + BKP * BMn;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;

    const int nwg = a.ktiles * a.ctiles * a.taps * a.splits;
    int bid = xcd_remap(blockIdx.x, nwg);
    const int split = bid / (a.ktiles * a.ctiles * a.taps);
    bid -= split * (a.ktiles * a.ctiles * a.taps);
    const int tap = bid / (a.ktiles * a.ctiles);
    bid -= tap * (a.ktiles * a.ctiles);
    const int kt_ = bid / a.ctiles, ct_ = bid - kt_ * a.ctiles;
    const int n0 = kt_ * BMn, c0 = ct_ * BNc;
    const int r = tap / a.kw, s = tap - r * a.kw;

    const int ych = tid % YCH, yrow = tid / YCH;
    const int xch = tid % XCH, xrow = tid / XCH;
    const bool y_ok = (n0 + ych * 4) < a.K;
    const bool x_ok = (c0 + xch * 4) < a.C;
    f32x4 mu = {0.f, 0.f, 0.f, 0.f}, sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
    if (PRO && x_ok) {
        mu = *reinterpret_cast<const f32x4*>(a.pro + c0 + xch * 4);
        sc = *reinterpret_cast<const f32x4*>(a.pro + a.C + c0 + xch * 4);
        sh = *reinterpret_cast<const f32x4*>(a.pro + 2 * a.C + c0 + xch * 4);
        if (BF16) sh -= mu * sc;      // one fma per element (see igemm_vec_kernel)
    }
    const int ohw = a.OH * a.OW;

    f32x4 ry[YP], rx[XP];
    unsigned x_valid = 0;
    // Loader without divisions (see igemm_vec_kernel: every vector instruction here is paid in matrix throughput): raw
    // buffer loads, dy rows at fixed per-lane offsets + a scalar pixel offset, and for x a (b, oh, ow) triple per loader
    // row that is decomposed once and then ADVANCED by the 64 pixels of a step with two carries.
    constexpr unsigned OOB = 0x80000000u;
    const bool x16 = a.x16 != 0, dy16 = a.dy16 != 0;
    const __amdgpu_buffer_rsrc_t rsrc_y =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.dy), 0, a.M * a.K * (dy16 ? 2 : 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_x =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, a.B * a.H * a.W * a.C * (x16 ? 2 : 4), 0x00020000);
    // pixel (within the step) of loader pass i: fp32 -- row + i * rows-per-pass; bf16 -- passes 2k, 2k+1 are ADJACENT pixels
    // (they share one 32-bit LDS word of the transposed tile)
    auto ypix = [&](int i) { return BF16 ? 2 * YRP * (i >> 1) + 2 * yrow + (i & 1) : yrow + i * YRP; };
    auto xpix = [&](int i) { return BF16 ? 2 * XRP * (i >> 1) + 2 * xrow + (i & 1) : xrow + i * XRP; };
    unsigned y_voff[YP];
#pragma unroll
    for (int i = 0; i < YP; ++i) y_voff[i] = y_ok ? (unsigned)(ypix(i) * a.K + n0 + ych * 4) * 4u : OOB;
    int xb[XP], xoh[XP], xow[XP];      // pixel of loader row i in the NEXT step to be loaded
    {
        const int p_first = (split * a.psteps_per_split) * BKP;
#pragma unroll
        for (int i = 0; i < XP; ++i) {
            const int p = p_first + xpix(i);
            xb[i] = p / ohw;
            const int rem = p - xb[i] * ohw;
            xoh[i] = rem / a.OW;
            xow[i] = rem - xoh[i] * a.OW;
        }
    }
    const int adv_b = BKP / ohw, adv_rem = BKP - adv_b * ohw;      // one step = adv_b images + adv_oh rows + adv_ow pixels
    const int adv_oh = adv_rem / a.OW, adv_ow = adv_rem - adv_oh * a.OW;
    const int x_lane = (c0 + xch * 4);
    auto load_tile = [&](int ps) {      // called once per step, in step order
        const int soff_y = ps * BKP * a.K * 4;
        if (dy16) {      // bf16 tensors: raw bits now, widened when the registers are consumed (see igemm_vec_kernel)
#pragma unroll
            for (int i = 0; i < YP; ++i) ld4_raw16(ry[i], rsrc_y, y_voff[i], soff_y);
        } else {
#pragma unroll
            for (int i = 0; i < YP; ++i) ry[i] = ld4(rsrc_y, y_voff[i], soff_y, false);
        }
        unsigned valid = 0;
        unsigned xoffs[XP];
#pragma unroll
        for (int i = 0; i < XP; ++i) {
            const int hi = xoh[i] * a.stride - a.pad + r, wi = xow[i] * a.stride - a.pad + s;
            const bool v = x_ok && xb[i] < a.B && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
            const unsigned e = ((((unsigned)xb[i] * a.H + hi) * a.W + wi) * a.C + x_lane) * 4u;      // garbage where !v
            xoffs[i] = v ? e : OOB;
            valid |= v ? (1u << i) : 0u;
            // advance to the next step's pixel
            int ow = xow[i] + adv_ow, oh = xoh[i] + adv_oh, b = xb[i] + adv_b;
            if (ow >= a.OW) { ow -= a.OW; ++oh; }
            if (oh >= a.OH) { oh -= a.OH; ++b; }
            xow[i] = ow; xoh[i] = oh; xb[i] = b;
        }
        if (x16) {
#pragma unroll
            for (int i = 0; i < XP; ++i) ld4_raw16(rx[i], rsrc_x, xoffs[i], 0);
        } else {
#pragma unroll
            for (int i = 0; i < XP; ++i) rx[i] = ld4(rsrc_x, xoffs[i], 0, false);
        }
        x_valid = valid;
    };
    // bf16 tiles: [channel][pixel], rows of WLD = 76 halfs (152 B = 38 words).  A lane owns 4 channels x 2 adjacent pixels
    // per pass pair = four 32-bit words in four rows; in the e-th of its four writes it takes channel (e + ych / 8) % 4, and
    // with the 38-word pitch the 64 lanes of a wave then hit 64 different banks (brute-forced; any plain order is 8-way
    // conflicted because the lanes of a wave differ in the CHANNEL chunk, i.e. by whole rows).
    constexpr int WLD = BMn == 128 ? 76 : 72;      // 64 x 64 tile (16 channel chunks per pixel row): 36 words, order (e + ych / 4) % 4
    constexpr int RSH = BMn == 128 ? 3 : 2;
    __bf16* Yh = reinterpret_cast<__bf16*>(smem);
    __bf16* Xh = Yh + BMn * WLD;
    auto rot4 = [](f32x4 v, int r) {      // v[(e + r) & 3] at position e, r per lane
        f32x4 t = (r & 1) ? f32x4{v[1], v[2], v[3], v[0]} : v;
        return (r & 2) ? f32x4{t[2], t[3], t[0], t[1]} : t;
    };
    auto store_pair = [&](__bf16* T, int ch, int rowp, f32x4 v0, f32x4 v1) {      // pixels 2 * rowp', 2 * rowp' + 1
        const int r = (ch >> RSH) & 3;
        const f32x4 a0 = rot4(v0, r), a1 = rot4(v1, r);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
            typedef float f32x2_ __attribute__((ext_vector_type(2)));
            f32x2_ v = {a0[e], a1[e]};
            __bf16* dst = &T[(ch * 4 + ((e + r) & 3)) * WLD + rowp];
            *reinterpret_cast<bf16x2*>(dst) = __builtin_convertvector(v, bf16x2);
        }
    };
    auto pro4 = [&](f32x4 v, int i) {
        if (PRO) {      // producer BN+ReLU applied after the MFMAs of the current step (see igemm_vec_kernel)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float t = BF16 ? fmaf(v[e], sc[e], sh[e]) : fmaf(v[e] - mu[e], sc[e], sh[e]);
                v[e] = a.pro_relu ? fmaxf(t, 0.f) : t;
            }
            if (!((x_valid >> i) & 1u)) v = f32x4{0.f, 0.f, 0.f, 0.f};      // padding / pixel tail: BN(0) != 0
        }
        return v;
    };
    auto unraw = [](f32x4 v) { return widen_bf16x4(u32x2{__float_as_uint(v[0]), __float_as_uint(v[1])}); };
    auto store_tile = [&]() {
        if (dy16) {
#pragma unroll
            for (int i = 0; i < YP; ++i) ry[i] = unraw(ry[i]);
        }
        if (x16) {
#pragma unroll
            for (int i = 0; i < XP; ++i) rx[i] = unraw(rx[i]);
        }
        if constexpr (BF16) {
#pragma unroll
            for (int i = 0; i < YP; i += 2) store_pair(Yh, ych, ypix(i), ry[i], ry[i + 1]);
#pragma unroll
            for (int i = 0; i < XP; i += 2) store_pair(Xh, xch, xpix(i), pro4(rx[i], i), pro4(rx[i + 1], i + 1));
        } else {
#pragma unroll
            for (int i = 0; i < YP; ++i)
                *reinterpret_cast<f32x4*>(&Ys[(yrow + i * YRP) * BMn + ych * 4]) = ry[i];
#pragma unroll
            for (int i = 0; i < XP; ++i)
                *reinterpret_cast<f32x4*>(&Xs[(xrow + i * XRP) * BNc + xch * 4]) = pro4(rx[i], i);
        }
    };

    f32x16 acc[RB][CB];
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
        for (int j = 0; j < CB; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

    const int ps_begin = split * a.psteps_per_split;
    const int ps_end = min(a.psteps, ps_begin + a.psteps_per_split);
    const float* y_frag = Ys + (lane >> 5) * BMn + wm * RB * 32 + (lane & 31);
    const float* x_frag = Xs + (lane >> 5) * BNc + wn * CB * 32 + (lane & 31);
    if (ps_begin < ps_end) {
        load_tile(ps_begin);
        store_tile();
    }
    __syncthreads();
    for (int ps = ps_begin; ps < ps_end; ++ps) {
        const bool more = ps + 1 < ps_end;
        if (more) load_tile(ps + 1);
        if constexpr (BF16) {      // 4 groups of 16 pixels; lane l: channel l % 32, pixels 8 * (l / 32) .. + 7 of the group
            const __bf16* yf = Yh + (wm * RB * 32 + (lane & 31)) * WLD + (lane >> 5) * 8;
            const __bf16* xf = Xh + (wn * CB * 32 + (lane & 31)) * WLD + (lane >> 5) * 8;
            auto frag8 = [](const __bf16* q) {      // rows are 8-byte, not 16-byte aligned (152-byte pitch): two b64 reads
                const bf16x4 lo = *reinterpret_cast<const bf16x4*>(q), hi = *reinterpret_cast<const bf16x4*>(q + 4);
                return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            };
            bf16x8 ay[2][RB], bx[2][CB];
            auto frags = [&](int set, int kg) {
#pragma unroll
                for (int i = 0; i < RB; ++i) ay[set][i] = frag8(yf + i * 32 * WLD + kg * 16);
#pragma unroll
                for (int j = 0; j < CB; ++j) bx[set][j] = frag8(xf + j * 32 * WLD + kg * 16);
            };
            frags(0, 0);
#pragma unroll
            for (int kg = 0; kg < BKP / 16; ++kg) {
                if (kg + 1 < BKP / 16) frags((kg + 1) & 1, kg + 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < RB; ++i)
#pragma unroll
                    for (int j = 0; j < CB; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ay[kg & 1][i], bx[kg & 1][j], acc[i][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {   // fragments of pixel pair kk+PF are read before the MFMAs of pair kk are issued (see igemm_vec_kernel)
            constexpr int PF = 2, NS = PF + 1;
            float av[NS][RB], bv[NS][CB];
            auto frags = [&](int set, int kk) {
#pragma unroll
                for (int i = 0; i < RB; ++i) av[set][i] = y_frag[kk * 2 * BMn + i * 32];
#pragma unroll
                for (int j = 0; j < CB; ++j) bv[set][j] = x_frag[kk * 2 * BNc + j * 32];
            };
#pragma unroll
            for (int q = 0; q < PF; ++q) frags(q, q);
#pragma unroll
            for (int kk = 0; kk < BKP / 2; ++kk) {
                if (kk + PF < BKP / 2) frags((kk + PF) % NS, kk + PF);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < RB; ++i)
#pragma unroll
                    for (int j = 0; j < CB; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kk % NS][i], bv[kk % NS][j], acc[i][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();
        if (more) store_tile();
        __syncthreads();
    }
    // epilogue: stage one wave-row of the tile at a time through LDS -> full 16-byte stores along c
    float* __restrict__ out = a.partial ? a.partial + (size_t)split * a.K * a.taps * a.C : a.dw;
    constexpr int RP = RB * 32;          // rows (n) per pass
    constexpr int LDC = BNc + 4;
    static_assert(RP * LDC <= BKP * (BMn + BNc), "wgrad epilogue staging does not fit the operand LDS");
    float* Cs = smem;
    for (int h = 0; h < WGM; ++h) {
        __syncthreads();
        if (wm == h) {
#pragma unroll
            for (int j = 0; j < CB; ++j)
#pragma unroll
                for (int i = 0; i < RB; ++i)
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int row = i * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
                        Cs[row * LDC + wn * CB * 32 + j * 32 + (lane & 31)] = acc[i][j][q];
                    }
        }
        __syncthreads();
        constexpr int C4 = BNc / 4;
        for (int idx = tid; idx < RP * C4; idx += 256) {
            const int row = idx / C4, c4 = idx - row * C4;
            const int n = n0 + h * RP + row, c = c0 + c4 * 4;
            if (n < a.K && c < a.C)
                *reinterpret_cast<f32x4*>(out + ((size_t)n * a.taps + tap) * a.C + c) =
                    *reinterpret_cast<const f32x4*>(&Cs[row * LDC + c4 * 4]);
        }
    }
}

// generic wgrad: flattened j = tap*C + c (any C); tile 64 (n) x 64 (j); waves 2 x 2
__global__ __launch_bounds__(256) void wgrad_gen_kernel(WgradArgs a) {
    constexpr int BMn = 64, BNj = 64;
    __shared__ __attribute__((aligned(16))) float smem[BK * (BMn + BNj)];
    float* Ys = smem;
    float* Xs = smem + BK * BMn;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int jtiles = a.ctiles;
    const int nwg = a.ktiles * jtiles * a.splits;
    int bid = xcd_remap(blockIdx.x, nwg);
    const int split = bid / (a.ktiles * jtiles);
    bid -= split * (a.ktiles * jtiles);
    const int kt_ = bid / jtiles, jt_ = bid - kt_ * jtiles;
    const int n0 = kt_ * BMn, j0 = jt_ * BNj;

    // thread -> column (n or j) and a group of 8 consecutive pixels
    const int col = tid & 63, pg = tid >> 6;
    const bool y_ok = (n0 + col) < a.K;
    const int j = j0 + col;
    const bool x_ok = j < a.J;
    const int tap = x_ok ? j / a.C : 0;
    const int c = x_ok ? j - tap * a.C : 0;
    const int r = tap / a.kw, s = tap - r * a.kw;
    const int ohw = a.OH * a.OW;

    float ry[8], rx[8];
    auto load_tile = [&](int ps) {
        const int p0 = ps * BK + pg * 8;
        int b = p0 / ohw;
        int rem = p0 - b * ohw;
        int oh = rem / a.OW, ow = rem - oh * a.OW;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int p = p0 + e;
            const bool pv = p < a.M;
            ry[e] = (y_ok && pv) ? a.dy[(size_t)p * a.K + n0 + col] : 0.f;
            const int hi = oh * a.stride - a.pad + r, wi = ow * a.stride - a.pad + s;
            const bool v = x_ok && pv && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
            rx[e] = v ? a.x[(((size_t)b * a.H + hi) * a.W + wi) * a.C + c] : 0.f;
            if (++ow == a.OW) {
                ow = 0;
                if (++oh == a.OH) {
                    oh = 0;
                    ++b;
                }
            }
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            Ys[(pg * 8 + e) * BMn + col] = ry[e];
            Xs[(pg * 8 + e) * BNj + col] = rx[e];
        }
    };
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    const int ps_begin = split * a.psteps_per_split;
    const int ps_end = min(a.psteps, ps_begin + a.psteps_per_split);
    const float* y_frag = Ys + (lane >> 5) * BMn + wm * 32 + (lane & 31);
    const float* x_frag = Xs + (lane >> 5) * BNj + wn * 32 + (lane & 31);
    if (ps_begin < ps_end) {
        load_tile(ps_begin);
        store_tile();
    }
    __syncthreads();
    for (int ps = ps_begin; ps < ps_end; ++ps) {
        const bool more = ps + 1 < ps_end;
        if (more) load_tile(ps + 1);
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(y_frag[kk * 2 * BMn], x_frag[kk * 2 * BNj], acc, 0, 0, 0);
        __syncthreads();
        if (more) store_tile();
        __syncthreads();
    }
    float* __restrict__ out = a.partial ? a.partial + (size_t)split * a.K * a.J : a.dw;
    const int jj = j0 + wn * 32 + (lane & 31);
    if (jj < a.J) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int n = n0 + wm * 32 + 4 * (lane >> 5) + (q & 3) + 8 * (q >> 2);
            if (n < a.K) out[(size_t)n * a.J + jj] = acc[q];
        }
    }
}

// Data gradient of a conv whose INPUT has <= 4 channels (the 7x7/2 stems behind the radar encoders' 6->3 adjust conv):
// as an implicit GEMM this has N = 3 (padded to a 32-wide tile) and, at stride 2, three of four taps invalid per pixel
// -- 2.5 TF.  Here one thread owns one input pixel, walks only the taps that reach it and dots dy's K channels
// (float4 loads) with the transposed weights held in LDS.  w_t is [C][taps][K]; K % 4 == 0; taps * C * K floats <= 40 KB.
template <int CIN>
__global__ __launch_bounds__(256) void thin_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w_t,
                                                         float* __restrict__ dx, int B, int H, int W, int OH, int OW,
                                                         int K, int kh, int kw, int stride, int pad, int accumulate) {
    extern __shared__ float wl[];      // [CIN][taps][K]
    const int taps = kh * kw, nw = CIN * taps * K;
    for (int i = threadIdx.x * 4; i < nw; i += 256 * 4) *reinterpret_cast<f32x4*>(wl + i) = *reinterpret_cast<const f32x4*>(w_t + i);
    __syncthreads();
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (int64_t)B * H * W) return;
    const int iw = (int)(pix % W), ih = (int)((pix / W) % H), b = (int)(pix / ((int64_t)W * H));
    float acc[CIN];
#pragma unroll
    for (int c = 0; c < CIN; ++c) acc[c] = 0.f;
    for (int r = (ih + pad) % stride; r < kh; r += stride) {
        const int oh = (ih + pad - r) / stride;
        if (ih + pad - r < 0 || oh >= OH) continue;
        for (int q = (iw + pad) % stride; q < kw; q += stride) {
            const int ow = (iw + pad - q) / stride;
            if (iw + pad - q < 0 || ow >= OW) continue;
            const float* g = dy + (((int64_t)b * OH + oh) * OW + ow) * K;
            const float* wt = wl + (r * kw + q) * K;
            for (int k = 0; k < K; k += 4) {
                const f32x4 gv = *reinterpret_cast<const f32x4*>(g + k);
#pragma unroll
                for (int c = 0; c < CIN; ++c) {
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(wt + c * taps * K + k);
                    acc[c] += gv[0] * wv[0] + gv[1] * wv[1] + gv[2] * wv[2] + gv[3] * wv[3];
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < CIN; ++c) {
        float* o = dx + pix * CIN + c;
        *o = accumulate ? *o + acc[c] : acc[c];
    }
}

// [K][taps][C] -> [C][taps][K]
__global__ void weight_transpose_kernel(const float* __restrict__ w, float* __restrict__ wt, int K,
                                        int taps, int C) {
    __shared__ float tile[32][33];
    const int tap = blockIdx.z;
    const int k0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    for (int i = ty; i < 32; i += 8) {
        const int k = k0 + i, c = c0 + tx;
        tile[i][tx] = (k < K && c < C) ? w[((size_t)k * taps + tap) * C + c] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, k = k0 + tx;
        if (c < C && k < K) wt[((size_t)c * taps + tap) * K + k] = tile[tx][i];
    }
}

// 64 x 64 tiles (all K, C of the batch multiples of 64): float4 reads along c, float4 writes along k (bf16: 8-byte writes),
// the transposition through a 65-float-pitch LDS tile -- 256-byte row segments on both sides instead of 128-byte ones and a
// quarter of the blocks (0.45 -> 0.25 ms per step for the 44.5 M camera weights)
__global__ __launch_bounds__(256) void weight_transpose_batch64_kernel(TransposeBatch tb) {
    __shared__ float tile[64 * 65];
    int i = 0;
    while (i + 1 < tb.n && (int)blockIdx.x >= tb.blk_start[i + 1]) ++i;      // wave-uniform scan (n <= 80)
    const int K = tb.K[i], taps = tb.taps[i], C = tb.C[i];
    const float* __restrict__ w = tb.w[i];
    float* __restrict__ wt = tb.wt[i];
    int rel = blockIdx.x - tb.blk_start[i];
    const int cb = C / 64, kb = K / 64;
    const int tap = rel / (cb * kb);
    rel -= tap * cb * kb;
    const int k0 = (rel / cb) * 64, c0 = (rel % cb) * 64;
    const int q = threadIdx.x & 15, r = threadIdx.x >> 4;      // 16 quads per row x 16 rows per pass
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int k = r + p * 16;
        const size_t idx = ((size_t)(k0 + k) * taps + tap) * C + c0 + q * 4;
        const f32x4 v = *reinterpret_cast<const f32x4*>(w + idx);
        if (tb.mode == 2) {
            *reinterpret_cast<bf16x4s*>(reinterpret_cast<__bf16*>(wt) + idx) = __builtin_convertvector(v, bf16x4s);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) tile[k * 65 + q * 4 + e] = v[e];
        }
    }
    if (tb.mode == 2) return;
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int c = r + p * 16;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = tile[(q * 4 + e) * 65 + c];
        const size_t o = ((size_t)(c0 + c) * taps + tap) * K + k0 + q * 4;
        if (tb.mode == 1) *reinterpret_cast<bf16x4s*>(reinterpret_cast<__bf16*>(wt) + o) = __builtin_convertvector(v, bf16x4s);
        else *reinterpret_cast<f32x4*>(wt + o) = v;
    }
}

// the same for up to 80 weight tensors in ONE launch (a ResNet stage's convs: 236 launches of ~5 us per step otherwise)
__global__ void weight_transpose_batch_kernel(TransposeBatch tb) {
    __shared__ float tile[32][33];
    int i = 0;
    while (i + 1 < tb.n && (int)blockIdx.x >= tb.blk_start[i + 1]) ++i;      // wave-uniform scan (n <= 80)
    const int K = tb.K[i], taps = tb.taps[i], C = tb.C[i];
    const float* __restrict__ w = tb.w[i];
    float* __restrict__ wt = tb.wt[i];
    int rel = blockIdx.x - tb.blk_start[i];
    const int cb = (C + 31) / 32, kb = (K + 31) / 32;
    const int tap = rel / (cb * kb);
    rel -= tap * cb * kb;
    const int k0 = (rel / cb) * 32, c0 = (rel % cb) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    for (int j = ty; j < 32; j += 8) {
        const int k = k0 + j, c = c0 + tx;
        const size_t idx = ((size_t)k * taps + tap) * C + c;
        const float v = (k < K && c < C) ? w[idx] : 0.f;
        tile[j][tx] = v;
        if (tb.mode == 2 && k < K && c < C) reinterpret_cast<__bf16*>(wt)[idx] = (__bf16)v;      // bf16 shadow, same order
    }
    if (tb.mode == 2) return;
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int c = c0 + j, k = k0 + tx;
        if (c < C && k < K) {
            const size_t o = ((size_t)c * taps + tap) * K + k;
            if (tb.mode == 1) reinterpret_cast<__bf16*>(wt)[o] = (__bf16)tile[tx][j];
            else wt[o] = tile[tx][j];
        }
    }
}

// db[k] += sum_m dy[m][k]; db zeroed by the launcher; K <= 256
__global__ void bias_grad_kernel(const float* __restrict__ dy, float* __restrict__ db, int64_t M, int K) {
    __shared__ float red[256];
    const int rpi = 256 / K;            // rows per iteration
    const int c = threadIdx.x % K, r0 = threadIdx.x / K;
    float s = 0.f;
    if (r0 < rpi)
        for (int64_t m = (int64_t)blockIdx.x * rpi + r0; m < M; m += (int64_t)gridDim.x * rpi)
            s += dy[m * K + c];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < K) {
        float t = 0.f;
        for (int i = 0; i < rpi; ++i) t += red[threadIdx.x + i * K];
        atomicAdd(&db[threadIdx.x], t);
    }
}

// The same column sums WITHOUT a cleared output and without atomics (round 4): every block leaves its K partial sums in a
// slab of the conv workspace (agent-scope stores), takes a ticket, and the block that draws the last one adds the partials
// in block order and writes db -- one launch, a fixed summation order.  kBiasBlocks blocks at most.
__global__ __launch_bounds__(256) void bias_grad_slab_kernel(const float* __restrict__ dy, float* __restrict__ db, int64_t M, int K,
                                                              float* __restrict__ slab, int* __restrict__ ticket) {
    __shared__ float red[256];
    __shared__ int last;
    const int rpi = 256 / K;            // rows per iteration
    const int c = threadIdx.x % K, r0 = threadIdx.x / K;
    float s = 0.f;
    if (r0 < rpi)
        for (int64_t m = (int64_t)blockIdx.x * rpi + r0; m < M; m += (int64_t)gridDim.x * rpi)
            s += dy[m * K + c];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < K) {
        float t = 0.f;
        for (int i = 0; i < rpi; ++i) t += red[threadIdx.x + i * K];
        __hip_atomic_store(slab + (size_t)blockIdx.x * K + threadIdx.x, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) last = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
    __syncthreads();
    if (!last) return;
    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // left clean
    float t = 0.f;
    if (r0 < rpi)
        for (int b = r0; b < (int)gridDim.x; b += rpi)
            t += __hip_atomic_load(slab + (size_t)b * K + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    red[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x < K) {
        float u = 0.f;
        for (int i = 0; i < rpi; ++i) u += red[threadIdx.x + i * K];
        db[threadIdx.x] = u;
    }
}

// ---------------------------------------------------------------------------------------------
// optional per-launch instrumentation (bench.py roofline): HIP events on the launch stream
// ---------------------------------------------------------------------------------------------
struct ProfRec {
    int kind;            // 0 fwd, 1 dgrad, 2 wgrad
    double flops;
    hipEvent_t e0, e1;
    int shape[7];        // B,H,W,C,K,k,stride
    int family;          // which pipe the launch ran on (kFam*), written by the dispatch code, not derived from the shape
};
static bool g_prof_on = false;
static bool g_serialize = false;                   // dpft_profile_serialize: one stream, no event brackets
bool profiling_active() { return g_prof_on || g_serialize; }   // resnet_plan: keep everything on one stream while timing
static std::vector<ProfRec> g_prof;

struct ProfScope {
    bool on;
    hipStream_t st;
    ProfRec r;
    int family = kFamVector;      // of the launch's plan (kFamVector: conv16, thin-channel, nothing launched)
    ProfScope(int kind, const dpft_conv_desc* d, hipStream_t s) : on(g_prof_on), st(s) {
        if (!on) return;
        r.kind = kind;
        r.flops = 2.0 * d->B * d->OH * d->OW * (double)d->K * d->kh * d->kw * d->C;
        const int sh[7] = {d->B, d->H, d->W, d->C, d->K, d->kh, d->stride};
        memcpy(r.shape, sh, sizeof(sh));
        (void)hipEventCreate(&r.e0);
        (void)hipEventCreate(&r.e1);
        (void)hipEventRecord(r.e0, st);
    }
    ~ProfScope() {
        if (!on) return;
        r.family = family;
        (void)hipEventRecord(r.e1, st);
        g_prof.push_back(r);
    }
};

}  // namespace dpft
#include "conv_pipe.h"
namespace dpft {

// ---- host side: what a launch will be is decided in conv_plan.h; here the process-wide mode, the arguments and the launches ----
static inline float* ws_slabs(void* workspace) { return workspace ? reinterpret_cast<float*>((char*)workspace + kWsHeader) : nullptr; }

// 0 = fp32 MFMA (the reference's arithmetic), 1 = bf16 operands / fp32 accumulation in the forward and data-gradient
// GEMMs of the C % 64 == 0 convs (BASELINE.json configs[4], "bf16 mixed precision"); process-wide, set between launches
static int g_conv_bf16 = tuning().compute0;
// fp32 mode: the big multi-tap GEMMs (3x3 / 7x7 filters over C % 64 == 0 channels, >= 2 GFLOP) run as 3 x bf16 split products on
// the bf16 matrix cores (conv_x3.hip) -- fp32 operands, fp32 results, error against fp64 BELOW the fp32 MFMA's on every
// shape of the step (tests/test_gpu_conv_table.py).  dpft_conv_set_split(0) / DPFT_CONV_SPLIT=0: fp32 MFMA everywhere.
static int g_conv_split = tuning().split0;
static PlanMode plan_mode() { return PlanMode{g_conv_bf16, g_conv_bf16 == 2 || (g_conv_bf16 == 0 && g_conv_split)}; }

static void fill_igemm(IgemmArgs& a, const dpft_conv_desc* d, bool dgrad) {
    memset(&a, 0, sizeof(a));
    const GemmDims g = gemm_dims(d, dgrad);
    a.kh = d->kh; a.kw = d->kw; a.stride = d->stride; a.pad = d->pad;
    a.B = d->B; a.C = g.C; a.N = g.N; a.M = g.M; a.Ktot = g.Ktot; a.ksteps = g.ksteps;
    a.H = dgrad ? d->OH : d->H; a.W = dgrad ? d->OW : d->W;
    a.OH = dgrad ? d->H : d->OH; a.OW = dgrad ? d->W : d->OW;
    a.x16 = a.y16 = d->act16 != 0;
}
// split-K slabs and tickets of a planned launch (the workspace was required by the entry)
static void set_split(IgemmArgs& a, const IgemmPlan& p, void* workspace) {
    if (p.splits > 1) a.partial = ws_slabs(workspace);
    if (p.fixup) a.sk_ticket = reinterpret_cast<int*>(workspace);      // the last split workgroup of a tile runs the whole epilogue
}

// launch with dynamic LDS; raises the per-kernel dynamic-LDS cap once (tiles above 64 KiB)
template <typename K, typename A>
static void launch_lds(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, const A& args) {
    static LdsGrant grant;      // one per kernel instantiation: the largest size allowed so far, per device
    (void)lds_grant(grant, reinterpret_cast<const void*>(kernel), lds);
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args);
}

// Launches the kernel the plan names, on the tile the plan names; decides nothing.
template <bool DGRAD>
static int launch_igemm(IgemmArgs& a, const IgemmPlan& p, bool pro, hipStream_t st) {
    if (p.vec) {      // the vector loader keeps a 32-bit tap mask per row and 32-bit buffer offsets
        DPFT_REQUIRE(a.kh <= 8 && a.kw <= 8, "conv: the C %% 64 == 0 path supports filters up to 8x8 (%dx%d)", a.kh, a.kw);
        DPFT_REQUIRE((int64_t)a.B * a.H * a.W * a.C < (1ll << 29) && (int64_t)a.N * a.Ktot < (1ll << 29),
                     "conv: operand larger than 2 GiB");
    }
    static const int ablate_env = getenv("DPFT_ABLATE") ? atoi(getenv("DPFT_ABLATE")) : 0;
    a.ablate = ablate_env;
    a.epf = p.epf;
    a.mtiles = cdiv(a.M, p.bm); a.ntiles = cdiv(a.N, p.bn); a.splits = p.splits;
    a.ksteps = a.ksteps * BKV / p.pbk;      // (a parity class of a strided data gradient covers a subset of the taps)
    a.ksteps_per_split = cdiv(a.ksteps, a.splits);
    DPFT_REQUIRE(!p.fixup || a.mtiles * a.ntiles <= kWsTickets, "conv: %d output tiles exceed the split-K ticket header", a.mtiles * a.ntiles);
    const dim3 grid(a.mtiles * a.ntiles * a.splits), block(256), block2(512);
    // (any other tile runs 64 x 64)
    const int tile = ((p.bm == 128 && (p.bn == 128 || p.bn == 64)) || (p.bm == 64 && p.bn == 128)) ? p.bm * 1000 + p.bn : 64064;
#define PIPE_LDS(BM_, BN_, PBK_, ES_) std::max((size_t)2 * (BM_ + BN_) * PBK_ * ES_, (size_t)BM_ * (BN_ + 4) * 4 + (size_t)3 * BN_ * 4)
#define GO_PIPE(BM_, BN_, PBK_, PRO_, B16_, EPF_)                                                          \
    launch_lds(igemm_pipe_kernel<BM_, BN_, 2, 2, PBK_, DGRAD, PRO_, B16_, EPF_>, grid, block,              \
               PIPE_LDS(BM_, BN_, PBK_, (B16_ ? 2 : 4)) + (PRO_ ? (size_t)12 * a.C : 0), st, a)
// one instantiation of igemm_pipe_kernel, taken where the plan names its tile, K-step and prefetch mode (EpiPrefetch: modes 1, 2 exist
// for data gradients, 3 for the forward); the operand prologue exists in the plain fp32 forward
#define PIPE(BM_, BN_, PBK_, B16_, EPF_)                                                                   \
    if constexpr (EPF_ == 0 || (EPF_ == 3) != DGRAD)                                                       \
        if (tile == BM_ * 1000 + BN_ && p.pbk == PBK_ && p.epf_kernel == EPF_) {                           \
            if constexpr (!DGRAD && !B16_ && EPF_ == 0)                                                    \
                if (pro) { GO_PIPE(BM_, BN_, PBK_, true, false, 0); break; }                               \
            GO_PIPE(BM_, BN_, PBK_, false, B16_, EPF_);                                                    \
            break;                                                                                         \
        }
    switch (p.kernel) {
    case kAllTap:
        if constexpr (DGRAD) launch_lds(igemm_vec_kernel<64, 64, 2, 2, true, false, false>, grid, block, (size_t)(64 + 64) * LDK * sizeof(float), st, a);
        return check_launch("conv igemm (strided dgrad, all taps)");
    case kB16w: return launch_igemm_b16w(a, p.bm, p.bn, DGRAD, st);      // conv_b16w.hip: 256-row tiles, eight waves
    case kX3Planes: return launch_igemm_x3(a, p.bm, p.bn, DGRAD, false, false, st);
    case kX3: return launch_igemm_x3(a, p.bm, p.bn, DGRAD, pro, p.row3, st);
    case kPipe16:      // everything by LDS-DMA, 2-byte elements
        PIPE(128, 64, 64, true, 1) PIPE(128, 64, 64, true, 2) PIPE(64, 64, 128, true, 2) PIPE(64, 64, 64, true, 2)
        PIPE(128, 128, 64, true, 0) PIPE(128, 64, 64, true, 0) PIPE(64, 64, 128, true, 0) PIPE(64, 64, 64, true, 0)
        DPFT_REQUIRE(false, "conv igemm: no pipelined bf16 kernel for the planned tile");
    case kPipe:      // (64 x 64 with 32-wide K-steps: 32 KB of LDS, more resident workgroups to overlap prologues / epilogues)
        PIPE(128, 64, 32, false, 1) PIPE(128, 64, 32, false, 2) PIPE(64, 64, 64, false, 2)
        PIPE(128, 128, 32, false, 3) PIPE(128, 64, 32, false, 3) PIPE(64, 64, 64, false, 3)
        PIPE(128, 128, 32, false, 0) PIPE(128, 64, 32, false, 0) PIPE(64, 128, 32, false, 0) PIPE(64, 64, 32, false, 0) PIPE(64, 64, 64, false, 0)
        DPFT_REQUIRE(false, "conv igemm: no pipelined kernel for the planned tile");
    case kVec:
    case kVecKS2: {
        const bool ks2 = p.kernel == kVecKS2, b16 = p.family == kFamBf16;
#define LAUNCH_VEC(BM_, BN_)                                                                  \
    do {                                                                                      \
        constexpr size_t lds = (size_t)(BM_ + BN_) * LDK * sizeof(float);                     \
        if (ks2) {                                                                            \
            if constexpr (DGRAD && BM_ == 64 && BN_ == 64) {                                  \
                if (b16) launch_lds(igemm_vec_kernel<BM_, BN_, 2, 2, true, false, true, true, 2>, grid, block2, lds, st, a);       \
                else launch_lds(igemm_vec_kernel<BM_, BN_, 2, 2, true, false, true, false, 2>, grid, block2, lds, st, a);          \
            }                                                                                 \
        } else if (b16) {                                                                     \
            if (pro) launch_lds(igemm_vec_kernel<BM_, BN_, 2, 2, DGRAD, !DGRAD, true, true>, grid, block, lds, st, a); \
            else launch_lds(igemm_vec_kernel<BM_, BN_, 2, 2, DGRAD, false, true, true>, grid, block, lds, st, a);      \
        } else if (pro) launch_lds(igemm_vec_kernel<BM_, BN_, 2, 2, DGRAD, !DGRAD>, grid, block, lds, st, a); \
        else launch_lds(igemm_vec_kernel<BM_, BN_, 2, 2, DGRAD, false>, grid, block, lds, st, a);      \
    } while (0)
        if (tile == 128128) LAUNCH_VEC(128, 128);
        else if (tile == 128064) LAUNCH_VEC(128, 64);
        else LAUNCH_VEC(64, 64);
#undef LAUNCH_VEC
        break;
    }
    default:      // kGeneric
        if (p.bn == 32) hipLaunchKernelGGL((igemm_gen_kernel<32, DGRAD>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((igemm_gen_kernel<64, DGRAD>), grid, block, 0, st, a);
        break;
    }
#undef PIPE
#undef GO_PIPE
#undef PIPE_LDS
    return check_launch("conv igemm");
}

}  // namespace dpft
#include "conv16_kernels.h"
namespace dpft {

// thin-channel weight gradients (conv16_kernels.h) as planned: p.blocks slabs in the workspace, then the slab reduction
// `db`: the bias gradient sum_p dy[p][k], carried where p.reduce == kWgReduceSlabBias
static int thin_wgrad(const dpft_conv_desc* d, const WgradPlan& p, const float* x, const float* dy, float* dw, float* db, void* workspace,
                      hipStream_t st) {
    float* slabs = ws_slabs(workspace);      // the slabs start behind the ticket header
    const bool with_bias = p.reduce == kWgReduceSlabBias;
    const dim3 grid(p.blocks), block(256);
    const long M = (long)d->B * d->H * d->W;
    int n = d->K * d->C, cols = 0;      // floats of dw; bias sums: column `cols` of every row (thin 1x1), or behind the n floats (cols = 0)
    switch (p.kernel) {
    case kWgConv16Tiled: {
        Wgrad16TArgs a{x, dy, slabs, d->B, d->H, d->W, cdiv(d->W, T16W), cdiv(d->H, T16H), d->B * cdiv(d->H, T16H) * cdiv(d->W, T16W), with_bias ? 1 : 0};
        hipLaunchKernelGGL(wgrad16_3x3_tiled_kernel, grid, block, 0, st, a);
        n = 2304;
        break;
    }
    case kWgConv16: {
        Wgrad16Args a{x, dy, slabs, d->B, d->H, d->W, cdiv(d->W, 4), (long)d->B * d->H * cdiv(d->W, 4)};
        hipLaunchKernelGGL(wgrad16_3x3_kernel, grid, block, 0, st, a);
        n = 2304;
        break;
    }
    case kWgStem7: {
        const int tw = cdiv(d->OW, STEM_OW), th = cdiv(d->OH, STEM_OH);
        WgradStemArgs a{x, dy, slabs, d->B, d->H, d->W, d->OH, d->OW, tw, th, d->B * th * tw};
        hipLaunchKernelGGL(wgrad_stem7_kernel, grid, block, 0, st, a);
        n = 64 * 147;
        break;
    }
    default:      // kWgThin1x1; with the bias gradient as a virtual input channel of ones
        cols = d->C + 1;
        if (d->K == 3) hipLaunchKernelGGL((wgrad1x1_small_kernel<3, 6>), grid, block, 0, st, x, dy, slabs, M);
        else if (d->C == 3 && with_bias) hipLaunchKernelGGL((wgrad1x1_k16_kernel<3, true>), grid, block, 0, st, x, dy, slabs, M);
        else if (with_bias) hipLaunchKernelGGL((wgrad1x1_k16_kernel<6, true>), grid, block, 0, st, x, dy, slabs, M);
        else if (d->C == 3) hipLaunchKernelGGL((wgrad1x1_k16_kernel<3>), grid, block, 0, st, x, dy, slabs, M);
        else hipLaunchKernelGGL((wgrad1x1_k16_kernel<6>), grid, block, 0, st, x, dy, slabs, M);
    }
    int rc = check_launch("thin wgrad");
    if (rc) return rc;
    const int nb = cols ? 16 * cols : kConv16Slab;      // floats per slab with the bias sums
    if (with_bias) hipLaunchKernelGGL(slab_reduce_bias_kernel, dim3(cdiv(nb, 16)), block, 0, st, (const float*)slabs, dw, db, nb, p.blocks, cols, cols ? 0 : n);
    else hipLaunchKernelGGL(slab_reduce_kernel, dim3(cdiv(n, 16)), block, 0, st, (const float*)slabs, dw, n, p.blocks);
    return check_launch("thin wgrad reduce");
}

static int check_desc(const dpft_conv_desc* d) {
    DPFT_REQUIRE(d != nullptr, "conv: null descriptor");
    DPFT_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->K > 0, "conv: non-positive dims");
    DPFT_REQUIRE(d->kh > 0 && d->kw > 0 && d->stride > 0 && d->pad >= 0, "conv: bad filter geometry");
    const int oh = (d->H + 2 * d->pad - d->kh) / d->stride + 1;
    const int ow = (d->W + 2 * d->pad - d->kw) / d->stride + 1;
    DPFT_REQUIRE(oh == d->OH && ow == d->OW, "conv: OH/OW (%d,%d) inconsistent with geometry (%d,%d)",
                 d->OH, d->OW, oh, ow);
    DPFT_REQUIRE((int64_t)d->B * d->H * d->W * d->C < (1ll << 31) &&
                 (int64_t)d->B * d->OH * d->OW * d->K < (1ll << 31), "conv: tensor too large for 32-bit row indices");
    DPFT_REQUIRE(d->act16 >= 0 && d->act16 <= 2, "conv: act16 must be 0, 1 or 2 (is the descriptor zero-initialised?)");
    // bf16 activation storage rides on the vector loaders / the staged epilogue only
    DPFT_REQUIRE(!d->act16 || (d->C % BKV == 0 && d->K % BKV == 0 && d->kh <= 8 && d->kw <= 8),
                 "conv: act16 (bf16 activation storage) needs C %% 64 == 0 and K %% 64 == 0 (C=%d, K=%d)", d->C, d->K);
    return DPFT_OK;
}

}  // namespace dpft

using namespace dpft;

// Worst case over the slabs of every form of the problem: the contract's BOUNDS, not one plan's slabs (the plans never ask for more)
extern "C" int64_t dpft_conv2d_workspace_bytes(const dpft_conv_desc* d) {
    if (check_desc(d) != DPFT_OK) return -1;
    int64_t best = 0;
    if (conv16_matches(d)) best = std::max<int64_t>(best, (int64_t)conv16_wgrad_blocks(d) * kConv16Slab * 4);      // (both forms, + bias column sums)
    if (d->kh == 1 && d->kw == 1 && d->K <= 16 && d->C <= 8) best = std::max<int64_t>(best, (int64_t)kNumCU * 2 * d->K * (d->C + 1) * 4);      // thin 1x1: blocks <= 2 per CU
    const ForceTile force;
    for (bool split_on : {false, true})      // with or without the split kernels, whichever the launches will run with
        for (bool dgrad : {false, true}) {
            const GemmDims g = gemm_dims(d, dgrad);
            TileChoice t = choose_tile(g.M, g.N, g.C, g.ksteps, d->act16 ? 1 : taps_of(d), PlanMode{g_conv_bf16, split_on}, force);
            if (d->act16) t.splits = 1;
            (void)big16_tile(d, g, dgrad, true, force, t);
            if (t.splits > 1) best = std::max<int64_t>(best, (int64_t)t.splits * g.M * g.N * 4);
        }
    const int64_t wbytes = (int64_t)d->K * d->kh * d->kw * d->C * 4;      // wgrad: pixel-split partial slabs
    best = std::max<int64_t>(best, wgrad_max_splits(wbytes) * wbytes);
    best = std::max<int64_t>(best, (int64_t)kBiasBlocks * std::min(d->K, 256) * 4);      // bias_grad_slab_kernel's partial sums
    return best + (int64_t)kWsHeader;
}

extern "C" int64_t dpft_conv2d_workspace_header_bytes(void) { return (int64_t)kWsHeader; }

extern "C" int dpft_conv2d_workspace_init(void* workspace, dpft_stream_t stream) {
    DPFT_REQUIRE(workspace, "conv2d_workspace_init: null workspace");
    return dpft::zero_fill(workspace, kWsHeader, stream);
}

extern "C" int dpft_split_planes_f32(const float* src, void* planes, int64_t n, dpft_stream_t stream) {
    return dpft::split_planes(src, planes, n, (hipStream_t)stream);
}

extern "C" int dpft_conv_set_compute(int32_t mode) {
    DPFT_REQUIRE(mode >= 0 && mode <= 2, "conv_set_compute: mode 0 (fp32), 1 (bf16 operands) or 2 (3 x bf16 split), got %d", mode);
    dpft::g_conv_bf16 = mode;
    return DPFT_OK;
}

extern "C" int32_t dpft_conv_get_compute() { return dpft::g_conv_bf16; }

extern "C" int dpft_conv_set_split(int32_t on) {
    dpft::g_conv_split = on != 0;
    return DPFT_OK;
}

extern "C" int32_t dpft_conv_get_split() { return dpft::g_conv_split; }

int dpft::conv_mode_key() { return dpft::g_conv_bf16 * 2 + (dpft::g_conv_split ? 1 : 0); }

// The statistics tiling = the tile rows of the forward plan with statistics wanted.  The query does not know the prologue: a
// multi-tap conv of >= 2 GFLOP in a split-on mode with a prologue WITHOUT ReLU is planned with `taps = 1` by conv_fwd_sums and
// may get another tile height than the one reported here.  No caller in the repository passes that prologue with statistics.
extern "C" int32_t dpft_conv2d_stats_tiles(const dpft_conv_desc* d, int32_t* tile_rows) {
    if (check_desc(d) != DPFT_OK) return -1;
    IgemmIn in;
    in.stats = true;
    const IgemmPlan p = plan_igemm(d, kFwd, in, plan_mode());
    if (tile_rows) *tile_rows = p.bm;
    return cdiv((int64_t)d->B * d->OH * d->OW, p.bm);
}

bool dpft::conv_fwd_pro_from_sums(const dpft_conv_desc* d) {
    IgemmIn in;
    in.ws = in.pro = in.pro_relu = in.stats = in.sums = true;
    return plan_igemm(d, kFwd, in, plan_mode()).pro_from_sums;
}

// family of the last launch a strided data gradient makes as parity classes (what its profile record holds)
static int classes_family(const dpft_conv_desc* d, const IgemmIn& in, const PlanMode& mode) {
    int family = kFamVector;
    for (int ph = 0; ph < d->stride; ++ph)
        for (int pw = 0; pw < d->stride; ++pw) {
            DgradClass c;
            if (!dgrad_class(d, ph, pw, c)) continue;
            IgemmIn q = in;
            q.M = c.M; q.ksteps = c.ksteps;
            family = plan_igemm(d, kDgradClass, q, mode).family;
        }
    return family;
}

extern "C" int32_t dpft_conv2d_planned_family(const dpft_conv_desc* d, int32_t kind, int32_t has_workspace) {
    if (check_desc(d) != DPFT_OK || kind < 0 || kind > 2) return -1;
    if (kind == 2) {
        WgradIn in;
        in.ws = has_workspace != 0;
        return plan_wgrad(d, in, plan_mode()).family;
    }
    IgemmIn in;
    in.ws = has_workspace != 0;
    const IgemmPlan p = plan_igemm(d, kind == 0 ? kFwd : kDgrad, in, plan_mode());
    return p.kernel == kClasses ? classes_family(d, in, plan_mode()) : p.family;
}

extern "C" int dpft_conv2d_nhwc_fwd_f32(const dpft_conv_desc* d, const float* x, const float* w,
                                        const float* bias, const float* pro_bn, int32_t pro_relu,
                                        float* y, float* stats, void* workspace, dpft_stream_t stream) {
    return dpft::conv_fwd_sums(d, x, w, bias, pro_bn, pro_relu, y, stats, workspace, stream);
}

int dpft::conv_fwd_sums(const dpft_conv_desc* d, const float* x, const float* w, const float* bias, const float* pro_bn,
                        int32_t pro_relu, float* y, float* stats, void* workspace, dpft_stream_t stream,
                        unsigned long long* sums, bool* sums_used, const BnSumsRef* pro_sums, bool* pro_sums_used) {
    if (sums_used) *sums_used = false;
    if (pro_sums_used) *pro_sums_used = false;
    if (pro_sums && !pro_sums->sums) pro_sums = nullptr;
    DPFT_REQUIRE(!pro_sums || (pro_bn && pro_sums_used), "conv fwd: a prologue from column sums needs the BN block's address and the answer slot");
    DPFT_REQUIRE(!sums || (stats && sums_used), "conv fwd: column sums need the statistics table and the answer slot");
    int rc = check_desc(d);
    if (rc) return rc;
    DPFT_REQUIRE(x && w && y, "conv fwd: null tensor");
    if (skip_conv("fwd3x3", "fwd1x1", d->kh, (int64_t)d->B * d->OH * d->OW)) return DPFT_OK;
    const bool pro = pro_bn != nullptr;
    IgemmIn in;
    in.ws = workspace != nullptr; in.bias = bias != nullptr; in.pro = pro; in.pro_relu = pro_relu != 0;
    in.stats = stats != nullptr; in.sums = sums != nullptr; in.planes = d->a_planes && d->w_planes;
    const IgemmPlan p = plan_igemm(d, kFwd, in, plan_mode());
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(0, d, st);
    prof.family = p.family;
    // statistics must come in the tiling dpft_conv2d_stats_tiles reports: no other kernel may take those of a streaming 1x1 shape
    DPFT_REQUIRE(!(p.stream_unfit && stats), "conv fwd: statistics of a streaming 1x1 conv (%d -> %d) take no bias and only the BatchNorm + ReLU prologue", d->C, d->K);
    DPFT_REQUIRE(!pro_sums || p.pro_from_sums, "conv fwd: the kernel of this conv builds no prologue from column sums (ask conv_fwd_pro_from_sums first)");
    if (p.stat_sums) *sums_used = true;      // column sums instead of the per-tile table; finalized by nobody here
    if (pro_sums) *pro_sums_used = true;
    if (p.kernel == kConv16) return conv16_forward(d, x, w, bias, y, st);
    if (p.kernel == kThin) return conv1x1_to16_forward(d, x, w, bias, y, st);
    if (p.kernel == kStream1x1) return launch_stream1x1(d, x, w, pro_bn, y, stats, nullptr, nullptr, 0, st, p.stat_sums ? sums : nullptr, pro_sums);
    DPFT_REQUIRE(!(d->act16 == 2 && (bias || pro_bn)), "conv fwd: act16 = 2 (bf16 weights) takes no bias and no operand prologue");
    DPFT_REQUIRE(!(pro && !p.vec), "conv fwd: fused prologue needs C %% 64 == 0 (C=%d)", d->C);
    DPFT_REQUIRE(p.splits == 1 || workspace, "conv fwd: split-K selected but no workspace given");
    IgemmArgs a; fill_igemm(a, d, false);
    a.x = x; a.w = w; a.y = y; a.bias = bias;
    a.pro = pro_bn; a.pro_relu = pro_relu;
    a.w16 = d->act16 == 2;
    if (p.kernel == kX3Planes) { a.x3 = d->a_planes; a.w3 = d->w_planes; }
    if (pro_sums) a.pro_s = *pro_sums;
    set_split(a, p, workspace);
    if (p.stat_sums) a.bns = sums;
    else if (p.splits == 1 || p.fixup) a.stats = stats;      // (a reduction launch produces them otherwise)
    rc = launch_igemm<false>(a, p, pro, st);
    if (rc || p.reduce == kReduceNone) return rc;
    const int64_t MN = (int64_t)a.M * a.N;
    if (p.reduce == kReduceStats) {      // reduce + per-tile (mean, M2) in one launch
        hipLaunchKernelGGL(splitk_reduce_stats_kernel, dim3(cdiv(a.M, p.bm), a.N / 64), dim3(256), 0, st, a.partial, y,
                           stats, (int64_t)a.M, a.N, p.splits, p.bm);
        return check_launch("conv fwd split-K reduce + stats");
    }
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3(cdiv(MN, 1024)), dim3(256), 0, st, a.partial, bias, y, MN, a.N, p.splits, 0);
    rc = check_launch("conv fwd split-K reduce");
    if (rc || !stats) return rc;
    return dpft_bn_stats_f32(y, stats, a.M, a.N, p.bm, stream);      // stats from the reduced output (p.bm rows per tile)
}

// C-ABI face of conv_fwd_sums (the launch plan's forward conv with its statistics / prologue as column sums): no arithmetic here
extern "C" int dpft_conv2d_nhwc_fwd_sums_f32(const dpft_conv_desc* d, const float* x, const float* w, const float* bias,
                                             const float* pro_bn, int32_t pro_relu, float* y, float* stats, uint64_t* sums,
                                             int32_t* sums_used, const uint64_t* pro_sums, const float* pro_gamma,
                                             const float* pro_beta, int64_t pro_rows, float pro_eps, int32_t* pro_sums_used,
                                             void* workspace, dpft_stream_t stream) {
    if (sums_used) *sums_used = 0;
    if (pro_sums_used) *pro_sums_used = 0;
    DPFT_REQUIRE(!pro_sums || (pro_gamma && pro_beta && pro_rows > 0 && pro_eps >= 0.f), "conv fwd (column sums): prologue sums without gamma / beta / rows / eps");
    const dpft::BnSumsRef ps{(const unsigned long long*)pro_sums, pro_gamma, pro_beta, pro_sums ? 1.0 / (double)pro_rows : 0.0, pro_eps, d ? d->C : 0};
    bool su = false, pu = false;
    const int rc = dpft::conv_fwd_sums(d, x, w, bias, pro_bn, pro_relu, y, stats, workspace, stream, (unsigned long long*)sums,
                                       sums_used ? &su : nullptr, pro_sums ? &ps : nullptr, pro_sums_used ? &pu : nullptr);
    if (sums_used) *sums_used = su ? 1 : 0;
    if (pro_sums_used) *pro_sums_used = pu ? 1 : 0;
    return rc;
}

// Inference form of conv + BatchNorm (+ residual) (+ ReLU): y = [relu](bn(conv(x, w)) [+ residual]) with the BN block of the
// OUTPUT channels.  One launch when the problem takes the vector path without split-K (the epilogue does it) or with the
// in-launch fix-up; otherwise the plain convolution followed by the elementwise pass -- same arithmetic, same result.
extern "C" int dpft_conv2d_nhwc_fwd_bnact_f32(const dpft_conv_desc* d, const float* x, const float* w, const float* out_bn,
                                              int32_t relu, const float* residual, float* y, void* workspace,
                                              dpft_stream_t stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    DPFT_REQUIRE(x && w && y && out_bn, "conv fwd_bnact: null tensor");
    // (the epilogue form and the elementwise pass both take the output channels four at a time; refused here, before the
    // convolution is launched, not by the pass behind it)
    DPFT_REQUIRE(d->K % 4 == 0, "conv fwd_bnact: K %% 4 == 0 needed (K=%d)", d->K);
    hipStream_t st = (hipStream_t)stream;
    IgemmIn in;
    in.ws = workspace != nullptr; in.residual = residual != nullptr; in.planes = d->a_planes && d->w_planes;
    const IgemmPlan p = plan_igemm(d, kFwdBnact, in, plan_mode());
    if (p.kernel == kTwoPass) {
        rc = dpft_conv2d_nhwc_fwd_f32(d, x, w, nullptr, nullptr, 0, y, nullptr, workspace, stream);
        if (rc) return rc;
        return bn_act_any(y, out_bn, residual, nullptr, relu, y, nullptr, (int64_t)d->B * d->OH * d->OW, d->K, d->act16 != 0, stream);
    }
    ProfScope prof(0, d, st);
    prof.family = p.family;
    if (p.kernel == kStream1x1) return launch_stream1x1(d, x, w, nullptr, y, nullptr, out_bn, residual, relu, st);
    IgemmArgs a; fill_igemm(a, d, false);
    a.x = x; a.w = w; a.y = y;
    if (p.kernel == kX3Planes) { a.x3 = d->a_planes; a.w3 = d->w_planes; }
    set_split(a, p, workspace);
    a.obn = out_bn; a.oadd = residual; a.orelu = relu;
    return launch_igemm<false>(a, p, false, st);
}

// One level of the FPN neck's forward as two launches (include/dpft_hip.h): the top-down add rides in the lateral's epilogue on
// the raw-input levels, the positional embedding in the 3x3 conv's; elsewhere conv + the elementwise kernel, same arithmetic.
extern "C" int dpft_fpn_lateral_f32(const dpft_conv_desc* d, const float* x, const float* w, const float* bias, const float* top,
                                    int32_t TH, int32_t TW, float* lat, void* workspace, dpft_stream_t stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    DPFT_REQUIRE(x && w && lat && d->kh == 1 && d->kw == 1 && d->stride == 1 && d->pad == 0, "fpn_lateral: a 1x1 conv (stride 1) with its tensors");
    DPFT_REQUIRE(!top || (TH >= 1 && TW >= 1 && TH <= d->H && TW <= d->W && d->K % 4 == 0), "fpn_lateral: bad top level (%d x %d)", TH, TW);
    if (top && tuning().fpn_fuse && conv1x1_to16_top_matches(d)) {
        ProfScope prof(0, d, (hipStream_t)stream);
        return conv1x1_to16_top_forward(d, x, w, bias, top, TH, TW, lat, (hipStream_t)stream);
    }
    rc = dpft_conv2d_nhwc_fwd_f32(d, x, w, bias, nullptr, 0, lat, nullptr, workspace, stream);
    if (rc || !top) return rc;
    return dpft_fpn_topdown_add_f32(lat, top, d->B, d->H, d->W, TH, TW, d->K, stream);
}

extern "C" int dpft_fpn_output_f32(const dpft_conv_desc* d, const float* lat, const float* w, const float* bias, const float* pos_x,
                                   const float* pos_y, float* out, void* workspace, dpft_stream_t stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    DPFT_REQUIRE(lat && w && out && (pos_x == nullptr) == (pos_y == nullptr), "fpn_output: null tensor / one embedding table without the other");
    DPFT_REQUIRE(d->H == d->OH && d->W == d->OW, "fpn_output: a same-size conv");
    if (pos_x && tuning().fpn_fuse && conv16_matches(d) && !d->act16) {
        ProfScope prof(0, d, (hipStream_t)stream);
        return conv16_forward(d, lat, w, bias, out, (hipStream_t)stream, pos_x, pos_y);
    }
    rc = dpft_conv2d_nhwc_fwd_f32(d, lat, w, bias, nullptr, 0, out, nullptr, workspace, stream);
    if (rc || !pos_x) return rc;
    return dpft_add_pos_f32(out, pos_x, pos_y, d->B, d->H, d->W, d->K, stream);
}

extern "C" int dpft_conv2d_nhwc_dgrad_f32(const dpft_conv_desc* d, const float* dy, const float* w_t,
                                          float* dx, int32_t accumulate, void* workspace,
                                          dpft_stream_t stream) {
    return dpft::conv_dgrad_fused(d, dy, w_t, dx, accumulate, workspace, stream, nullptr);
}

// the arguments both data-gradient entries share; the reduction `f` rides in the epilogue where the plan carries it
static void fill_dgrad(IgemmArgs& a, const dpft_conv_desc* d, const IgemmPlan& p, const float* dy, const float* w_t, float* dx, void* workspace,
                       dpft::BnReduceFuse* f) {
    fill_igemm(a, d, true);
    a.x = dy; a.w = w_t; a.y = dx;
    a.w16 = d->act16 == 2;
    if ((p.kernel == kX3Planes || p.kernel == kAllTap) && d->a_planes && d->w_planes && !d->act16) { a.x3 = d->a_planes; a.w3 = d->w_planes; }      // (kAllTap does not read them)
    set_split(a, p, workspace);
    if (!p.bnr) return;
    a.bnr_y = f->y; a.bnr_bnp = f->bnp; a.bnr_mask8 = f->mask8; a.bnr_self_mask = f->self_mask; a.bnr_sums = f->sums;
    f->applied = true;
}

// Data gradient with an optional fused BatchNorm-backward reduction (BnReduceFuse, common.h): `fuse->applied` tells the
// caller whether the launch(es) carried it -- split-K and thin-channel paths do not.
// With `res_src`: dx = dgrad(dy) + (res_mask > 0 ? res_src : 0), the stride-1 data gradient with the identity-branch ReLU
// backward folded into the epilogue (conv_dgrad_residual, used by the ResNet launch plan).
static int dgrad_any(const dpft_conv_desc* d, const float* dy, const float* w_t, float* dx, int32_t accumulate, bool res, const float* res_src,
                     const float* res_mask, const unsigned char* res_mask8, void* workspace, dpft_stream_t stream, dpft::BnReduceFuse* fuse) {
    if (fuse) fuse->applied = false;
    int rc = check_desc(d);
    if (rc) return rc;
    DPFT_REQUIRE(dy && w_t && dx && (!res || (res_src && res_mask)), "conv dgrad%s: null tensor", res ? " residual" : "");
    if (skip_conv("dgrad3x3", "dgrad1x1", d->kh, (int64_t)d->B * d->H * d->W)) {
        if (fuse && fuse->sums) fuse->applied = true;
        return DPFT_OK;
    }
    DPFT_REQUIRE(!res || (d->stride == 1 && !conv16_matches(d)), "conv dgrad residual: stride-1 bottleneck convs only");
    hipStream_t st = (hipStream_t)stream;
    IgemmIn in;
    in.ws = workspace != nullptr; in.accumulate = accumulate != 0; in.planes = d->a_planes && d->w_planes;
    in.bnr = fuse && fuse->sums && (d->C & 3) == 0;
    in.bnr_mask8 = res && fuse && fuse->mask8;
    in.res_mask8 = res && res_mask8 && (d->C & 3) == 0;      // (the split-K reduction and the scalar tail read res_mask)
    const IgemmPlan p = plan_igemm(d, res ? kDgradRes : kDgrad, in, plan_mode());
    ProfScope prof(1, d, st);
    prof.family = p.family;
    if (p.kernel == kConv16) return conv16_dgrad(d, dy, w_t, dx, accumulate, st);
    if (p.kernel == kThin) {
        const size_t lds = (size_t)d->C * d->kh * d->kw * d->K * 4;
        const dim3 grid(cdiv((int64_t)d->B * d->H * d->W, 256));
#define THIN_DGRAD(CI)                                                                                                  \
    hipLaunchKernelGGL(thin_dgrad_kernel<CI>, grid, dim3(256), lds, st, dy, w_t, dx, d->B, d->H, d->W, d->OH, d->OW, \
                       d->K, d->kh, d->kw, d->stride, d->pad, accumulate)
        switch (d->C) {
            case 1: THIN_DGRAD(1); break;
            case 2: THIN_DGRAD(2); break;
            case 3: THIN_DGRAD(3); break;
            default: THIN_DGRAD(4); break;
        }
#undef THIN_DGRAD
        return check_launch("conv dgrad (thin input)");
    }
    IgemmArgs a;
    if (p.kernel == kClasses) {
        // one launch per output-pixel parity class, each over the taps that can reach it (see IgemmArgs::sub_*)
        const int sp = d->stride;
        DgradClass c;
        bool empty_class = false;
        for (int ph = 0; ph < sp; ++ph)
            for (int pw = 0; pw < sp; ++pw)
                if (!dgrad_class(d, ph, pw, c) && (c.r0 >= d->kh || c.s0 >= d->kw)) empty_class = true;
        if (empty_class && !accumulate)      // pixels no tap reaches (1x1 stride-2: three of four) are plain zeros
            DPFT_REQUIRE(zero_fill(dx, (d->act16 ? 2 : sizeof(float)) * (size_t)d->B * d->H * d->W * d->C, st) == DPFT_OK,
                         "conv dgrad: zero fill failed");
        in.bnr = in.bnr && !empty_class;      // classes partition the pixels: every pixel is added once
        for (int ph = 0; ph < sp; ++ph)
            for (int pw = 0; pw < sp; ++pw) {
                if (!dgrad_class(d, ph, pw, c)) continue;
                in.M = c.M; in.ksteps = c.ksteps;
                const IgemmPlan q = plan_igemm(d, kDgradClass, in, plan_mode());
                fill_dgrad(a, d, q, dy, w_t, dx, workspace, fuse);
                a.accumulate = accumulate;
                a.sub_step = sp; a.sub_ph = ph; a.sub_pw = pw;
                a.sub_oh = c.oh; a.sub_ow = c.ow; a.sub_r0 = c.r0; a.sub_s0 = c.s0; a.sub_nr = c.nr; a.sub_ns = c.ns;
                a.M = c.M; a.ksteps = c.ksteps;
                prof.family = q.family;
                rc = launch_igemm<true>(a, q, false, st);
                if (rc) return rc;
            }
        return DPFT_OK;
    }
    DPFT_REQUIRE(p.splits == 1 || workspace, "conv dgrad: split-K selected but no workspace given");
    fill_dgrad(a, d, p, dy, w_t, dx, workspace, fuse);
    a.accumulate = accumulate;
    a.res_src = res_src; a.res_mask = res_mask;
    if (in.res_mask8) a.res_mask8 = res_mask8;
    rc = launch_igemm<true>(a, p, false, st);
    if (rc || p.reduce == kReduceNone) return rc;
    const int64_t MN = (int64_t)a.M * a.N;
    if (res) hipLaunchKernelGGL(splitk_reduce_residual_kernel, dim3(cdiv(MN, 256)), dim3(256), 0, st, a.partial, res_src, res_mask, dx, MN, p.splits);
    else hipLaunchKernelGGL(splitk_reduce_kernel, dim3(cdiv(MN, 1024)), dim3(256), 0, st, a.partial, (const float*)nullptr, dx, MN, a.N, p.splits, accumulate);
    return check_launch("conv dgrad split-K reduce");
}

int dpft::conv_dgrad_fused(const dpft_conv_desc* d, const float* dy, const float* w_t, float* dx, int32_t accumulate,
                           void* workspace, dpft_stream_t stream, BnReduceFuse* fuse) {
    return dgrad_any(d, dy, w_t, dx, accumulate, false, nullptr, nullptr, nullptr, workspace, stream, fuse);
}
int dpft::conv_dgrad_residual(const dpft_conv_desc* d, const float* dy, const float* w_t, float* dx, const float* res_src,
                              const float* res_mask, void* workspace, dpft_stream_t stream, BnReduceFuse* fuse,
                              const unsigned char* res_mask8) {
    return dgrad_any(d, dy, w_t, dx, 0, true, res_src, res_mask, res_mask8, workspace, stream, fuse);
}

// C-ABI face of the launch plan's fused data gradients (kernel-level parity: tests/test_gpu_conv_table.py)
extern "C" int dpft_conv2d_nhwc_dgrad_bn_reduce_f32(const dpft_conv_desc* d, const float* dy, const float* w_t, float* dx,
                                                    int32_t accumulate, const float* res_src, const float* res_out,
                                                    const uint8_t* res_mask8, const float* bn_y, const float* bn_block,
                                                    const uint8_t* bn_mask8, int32_t bn_self_mask, float* sums,
                                                    int32_t* applied, void* workspace, dpft_stream_t stream) {
    DPFT_REQUIRE(bn_y && bn_block && sums && applied, "conv dgrad_bn_reduce: null BatchNorm argument");
    DPFT_REQUIRE((bn_mask8 != nullptr) != (bn_self_mask != 0), "conv dgrad_bn_reduce: exactly one of bn_mask8 / bn_self_mask");
    dpft::BnReduceFuse f{bn_y, bn_block, bn_mask8, bn_self_mask, sums, false};
    int rc;
    if (res_src) {
        DPFT_REQUIRE(!accumulate && res_out, "conv dgrad_bn_reduce: the residual form needs res_out and does not accumulate");
        rc = dpft::conv_dgrad_residual(d, dy, w_t, dx, res_src, res_out, workspace, stream, &f, res_mask8);
    } else {
        rc = dpft::conv_dgrad_fused(d, dy, w_t, dx, accumulate, workspace, stream, &f);
    }
    *applied = f.applied ? 1 : 0;
    return rc;
}

// the planned weight gradient; `db` (may be null): the bias gradient too, *bias_done tells whether the launch carried it
static int launch_wgrad(const dpft_conv_desc* d, const float* x, const float* dy, const float* pro_bn, int32_t pro_relu, float* dw,
                        float* db, bool* bias_done, void* workspace, hipStream_t st) {
    const bool pro = pro_bn != nullptr;
    WgradIn in;
    in.ws = workspace != nullptr; in.pro = pro; in.pro_relu = pro_relu != 0; in.bias = db != nullptr;
    const WgradPlan p = plan_wgrad(d, in, plan_mode());
    ProfScope prof(2, d, st);
    prof.family = p.family;
    if (bias_done) *bias_done = p.reduce == kWgReduceSlabBias;
    if (p.blocks) return thin_wgrad(d, p, x, dy, dw, db, workspace, st);
    WgradArgs a; memset(&a, 0, sizeof(a));
    a.x = x; a.dy = dy; a.dw = dw; a.pro = pro_bn; a.pro_relu = pro_relu;
    a.x16 = a.dy16 = d->act16 != 0;
    a.B = d->B; a.H = d->H; a.W = d->W; a.C = d->C; a.OH = d->OH; a.OW = d->OW; a.K = d->K;
    a.kh = d->kh; a.kw = d->kw; a.stride = d->stride; a.pad = d->pad;
    a.M = d->B * d->OH * d->OW;
    a.taps = d->kh * d->kw;
    a.J = a.taps * a.C;
    DPFT_REQUIRE(!p.vec || ((int64_t)a.M * a.K < (1ll << 29) && (int64_t)a.B * a.H * a.W * a.C < (1ll << 29)),
                 "conv wgrad: operand larger than 2 GiB");
    a.ktiles = p.ktiles; a.ctiles = p.ctiles; a.splits = p.splits;
    a.psteps = cdiv(a.M, p.pk);
    a.psteps_per_split = cdiv(a.psteps, p.splits);
    a.partial = p.splits > 1 ? ws_slabs(workspace) : nullptr;
    const dim3 grid((int)(p.tiles * p.splits)), block(256);
    const size_t tbl = (size_t)a.psteps_per_split * p.pk * 4;      // pipelined forms: per-workgroup input-pixel offset table
    switch (p.kernel) {
    case kWgPipe16:
        if (p.bmn == 128) launch_lds(wgrad_pipe16_kernel<128, 128, 2, 2, 64>, grid, block, (size_t)2 * 64 * (128 + 128) * 2 + tbl, st, a);
        else launch_lds(wgrad_pipe16_kernel<64, 64, 2, 2, 128>, grid, block, (size_t)2 * 128 * (64 + 64) * 2 + tbl, st, a);
        break;
    case kWgX3: {
        int rc = launch_wgrad_x3(a, pro, grid, st);
        if (rc) return rc;
        break;
    }
    case kWgPipe:
        if (p.bmn == 128 && pro) launch_lds(wgrad_pipe_kernel<128, 128, 2, 2, 32, true>, grid, block, (size_t)2 * 32 * (128 + 128) * 4 + tbl, st, a);
        else if (p.bmn == 128) launch_lds(wgrad_pipe_kernel<128, 128, 2, 2, 32, false>, grid, block, (size_t)2 * 32 * (128 + 128) * 4 + tbl, st, a);
        else if (pro) launch_lds(wgrad_pipe_kernel<64, 64, 2, 2, 64, true>, grid, block, (size_t)2 * 64 * (64 + 64) * 4 + tbl, st, a);
        else launch_lds(wgrad_pipe_kernel<64, 64, 2, 2, 64, false>, grid, block, (size_t)2 * 64 * (64 + 64) * 4 + tbl, st, a);
        break;
    case kWgVec:
#define LAUNCH_WG(BM_, BN_, WGM_, WGN_, B16_)                                                           \
    do {                                                                                          \
        if (pro) hipLaunchKernelGGL((wgrad_vec_kernel<BM_, BN_, WGM_, WGN_, true, B16_>), grid, block, 0, st, a);  \
        else hipLaunchKernelGGL((wgrad_vec_kernel<BM_, BN_, WGM_, WGN_, false, B16_>), grid, block, 0, st, a);     \
    } while (0)
        if (p.bmn == 128 && p.family == kFamBf16) LAUNCH_WG(128, 128, 2, 2, true);      // mixed-precision mode: bf16 operands
        else if (p.bmn == 64 && p.family == kFamBf16) LAUNCH_WG(64, 64, 2, 2, true);
        else if (p.bmn == 128) LAUNCH_WG(128, 128, 2, 2, false);
        else if (p.bmn == 64) LAUNCH_WG(64, 64, 2, 2, false);
        else LAUNCH_WG(32, 128, 1, 4, false);
#undef LAUNCH_WG
        break;
    default:
        hipLaunchKernelGGL(wgrad_gen_kernel, grid, block, 0, st, a);
    }
    int rc = check_launch("conv wgrad");
    if (rc || p.reduce == kWgReduceNone || skip_family("wreduce")) return rc;      // (wreduce: the reduction launches' cost on the critical path)
    const int64_t n = (int64_t)d->K * a.J;
    if (p.reduce == kWgReduceWide16) hipLaunchKernelGGL(splitk_reduce_wide_kernel<16>, dim3(cdiv(n / 4, 16)), dim3(256), 0, st, a.partial, dw, n, p.splits);
    else if (p.reduce == kWgReduceWide4) hipLaunchKernelGGL(splitk_reduce_wide_kernel<4>, dim3(cdiv(n / 4, 64)), dim3(256), 0, st, a.partial, dw, n, p.splits);
    else hipLaunchKernelGGL(splitk_reduce_kernel, dim3(cdiv(n, 1024)), dim3(256), 0, st, a.partial, (const float*)nullptr, dw, n, 4, p.splits, 0);
    return check_launch("conv wgrad split-K reduce");
}

extern "C" int dpft_conv2d_nhwc_wgrad_f32(const dpft_conv_desc* d, const float* x, const float* dy,
                                          const float* pro_bn, int32_t pro_relu, float* dw,
                                          void* workspace, dpft_stream_t stream) {
    if (skip_family("wgrad")) return DPFT_OK;
    int rc = check_desc(d);
    if (rc) return rc;
    DPFT_REQUIRE(x && dy && dw, "conv wgrad: null tensor");
    DPFT_REQUIRE(!pro_bn || ((d->C % 32 == 0) && (d->K % 4 == 0)),
                 "conv wgrad: fused prologue needs C %% 32 == 0 and K %% 4 == 0 (C=%d, K=%d)", d->C, d->K);
    return launch_wgrad(d, x, dy, pro_bn, pro_relu, dw, nullptr, nullptr, workspace, (hipStream_t)stream);
}

extern "C" int dpft_weight_transpose_f32(const float* w, float* w_t, int32_t K, int32_t taps,
                                         int32_t C, dpft_stream_t stream) {
    DPFT_REQUIRE(w && w_t && K > 0 && taps > 0 && C > 0, "weight_transpose: bad arguments");
    dim3 grid(cdiv(C, 32), cdiv(K, 32), taps);
    hipLaunchKernelGGL(weight_transpose_kernel, grid, dim3(256), 0, (hipStream_t)stream, w, w_t, K, taps, C);
    return check_launch("weight_transpose");
}

extern "C" int dpft_weight_transpose_batch_f32(int32_t n, const float* const* w, float* const* w_t, const int32_t* K,
                                               const int32_t* taps, const int32_t* C, dpft_stream_t stream) {
    DPFT_REQUIRE(n >= 1 && n <= dpft::TransposeBatch::MAX && w && w_t && K && taps && C, "weight_transpose_batch: 1..80 tensors");
    dpft::TransposeBatch tb;
    tb.n = 0;
    tb.mode = 0;
    for (int i = 0; i < n; ++i) {
        DPFT_REQUIRE(w[i] && w_t[i] && K[i] > 0 && taps[i] > 0 && C[i] > 0, "weight_transpose_batch: bad entry %d", i);
        if (!tb.fits(K[i], C[i])) {      // tile edge of a launch (64 / 32): a second launch for the other kind
            int rc = dpft::weight_transpose_batch(tb, stream);
            if (rc) return rc;
            tb.n = 0;
        }
        tb.add(w[i], w_t[i], K[i], taps[i], C[i]);
    }
    return dpft::weight_transpose_batch(tb, stream);
}

int dpft::weight_transpose_batch(const TransposeBatch& tb, dpft_stream_t stream) {
    DPFT_REQUIRE(tb.n >= 1 && tb.n <= TransposeBatch::MAX, "weight_transpose_batch: 1..%d tensors", TransposeBatch::MAX);
    if (tb.tile == 64) hipLaunchKernelGGL(weight_transpose_batch64_kernel, dim3(tb.blk_start[tb.n]), dim3(256), 0, (hipStream_t)stream, tb);
    else hipLaunchKernelGGL(weight_transpose_batch_kernel, dim3(tb.blk_start[tb.n]), dim3(256), 0, (hipStream_t)stream, tb);
    return check_launch("weight_transpose_batch");
}

namespace dpft {
__global__ __launch_bounds__(256) void zero_fill_kernel(unsigned* __restrict__ p, size_t n4, size_t n) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) reinterpret_cast<uint4*>(p)[i] = uint4{0u, 0u, 0u, 0u};
    if (blockIdx.x == 0)
        for (size_t i = n4 * 4 + threadIdx.x; i < n; i += 256) p[i] = 0u;
}
}  // namespace dpft

int dpft::zero_fill(void* ptr, size_t bytes, dpft_stream_t stream) {
    DPFT_REQUIRE(ptr && (bytes & 3) == 0 && ((uintptr_t)ptr & 15) == 0, "zero_fill: 16-byte aligned pointer, size a multiple of 4");
    const size_t n = bytes / 4, n4 = n / 4;
    const int blocks = (int)std::max<size_t>(1, std::min<size_t>(kNumCU * 8, (n4 + 255) / 256));
    hipLaunchKernelGGL(zero_fill_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (unsigned*)ptr, n4, n);
    return check_launch("zero_fill");
}

extern "C" int dpft_bias_grad_f32(const float* dy, float* db, int64_t M, int32_t K,
                                  dpft_stream_t stream) {
    DPFT_REQUIRE(dy && db && M > 0 && K > 0 && K <= 256, "bias_grad: bad arguments (K=%d)", K);
    (void)hipMemsetAsync(db, 0, sizeof(float) * K, (hipStream_t)stream);
    const int rpi = 256 / K;
    int blocks = (int)std::min<int64_t>(1024, (M + rpi - 1) / rpi);
    hipLaunchKernelGGL(bias_grad_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dy, db, M, K);
    return check_launch("bias_grad");
}

// bias gradient behind a weight gradient on the same stream: the conv workspace is free again (ticket header zero, slabs
// consumed) -- the slab form above; without a workspace the cleared-output + atomics form
int dpft::bias_grad_ws(const float* dy, float* db, int64_t M, int32_t K, void* workspace, dpft_stream_t stream) {
    if (!workspace || !tuning().bias_slab || K > 256 || K <= 0) return dpft_bias_grad_f32(dy, db, M, K, stream);
    const int rpi = 256 / K;
    const int blocks = (int)std::min<int64_t>(kBiasBlocks, (M + rpi - 1) / rpi);
    hipLaunchKernelGGL(bias_grad_slab_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dy, db, M, (int)K, ws_slabs(workspace),
                       reinterpret_cast<int*>(workspace));
    return check_launch("bias_grad (slab)");
}

// Weight gradient AND bias gradient of a conv with bias (the FPN's convs): one pass over dy where the weight-gradient kernel
// has dy at hand (3x3 16 -> 16, thin 1x1 -> 16), the two separate launches otherwise.  Same results either way.
extern "C" int dpft_conv2d_nhwc_wgrad_bias_f32(const dpft_conv_desc* d, const float* x, const float* dy, float* dw, float* db,
                                               void* workspace, dpft_stream_t stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    DPFT_REQUIRE(x && dy && dw && db, "conv wgrad_bias: null tensor");
    // the thin kernels that have dy at hand (3x3 16 -> 16, thin 1x1 -> 16) carry the bias gradient (DPFT_SKIP=wgrad leaves them in)
    const bool fuse = tuning().bias_fuse && workspace && !d->act16 && (conv16_matches(d) || conv1x1_to16_top_matches(d));
    bool bias_done = false;
    if (fuse || !skip_family("wgrad")) rc = launch_wgrad(d, x, dy, nullptr, 0, dw, fuse ? db : nullptr, &bias_done, workspace, (hipStream_t)stream);
    if (rc || bias_done) return rc;
    return dpft::bias_grad_ws(dy, db, (int64_t)d->B * d->OH * d->OW, d->K, workspace, stream);
}

static float g_prof_overhead_ms = 0.f;      // elapsed time of an EMPTY event bracket (subtracted from every record)

extern "C" int dpft_profile_start(void) {
    for (auto& r : g_prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    g_prof.clear();
    // calibrate the bracket itself: two back-to-back event records cost a few us of queue time that is not the
    // kernel's (rocprofv3's per-kernel durations do not contain it)
    {
        hipStream_t st;
        if (hipStreamCreate(&st) == hipSuccess) {
            float samples[15];
            int n = 0;
            for (int i = 0; i < 15; ++i) {
                hipEvent_t a, b;
                if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) break;
                (void)hipEventRecord(a, st);
                (void)hipEventRecord(b, st);
                float ms = 0.f;
                if (hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&ms, a, b) == hipSuccess) samples[n++] = ms;
                (void)hipEventDestroy(a);
                (void)hipEventDestroy(b);
            }
            (void)hipStreamDestroy(st);
            if (n > 0) {
                std::sort(samples, samples + n);
                g_prof_overhead_ms = samples[n / 2];
            }
        }
    }
    g_prof_on = true;
    return DPFT_OK;
}

extern "C" float dpft_profile_overhead_ms(void) { return g_prof_overhead_ms; }

extern "C" int dpft_profile_serialize(int32_t on) {
    g_serialize = on != 0;
    return DPFT_OK;
}

extern "C" int32_t dpft_profile_stop(void) {
    g_prof_on = false;
    return (int32_t)g_prof.size();
}

extern "C" int dpft_profile_get_family(int32_t i, int32_t* family) {
    DPFT_REQUIRE(i >= 0 && i < (int32_t)g_prof.size() && family, "profile_get_family: bad index");
    *family = g_prof[i].family;
    return DPFT_OK;
}

extern "C" int dpft_profile_get(int32_t i, int32_t* kind, double* flops, float* ms, int32_t* shape7) {
    DPFT_REQUIRE(i >= 0 && i < (int32_t)g_prof.size() && kind && flops && ms && shape7, "profile_get: bad index");
    const ProfRec& r = g_prof[i];
    *kind = r.kind;
    *flops = r.flops;
    if (hipEventElapsedTime(ms, r.e0, r.e1) != hipSuccess) {
        set_error("profile_get: events not complete (synchronise the stream first)");
        return DPFT_ERR_LAUNCH;
    }
    *ms = fmaxf(*ms - g_prof_overhead_ms, 0.f);
    memcpy(shape7, r.shape, sizeof(r.shape));
    return DPFT_OK;
}
