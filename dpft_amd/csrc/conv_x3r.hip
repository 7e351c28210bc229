// The row-shared main loop of the 3 x bf16 split implicit GEMM (conv_x3.hip explains the split and the loop this one derives from).
#include "conv_core.h"

namespace dpft {

// ---------------------------------------------------------------------------------------------------------------------
// The 3x3 / stride 1 / pad 1 form of igemm_x3_kernel with the A tile staged once per FILTER ROW.  The three taps of a filter row
// read the same pixels shifted by one, and in igemm_x3_kernel's loop each of them loads, BatchNorm + ReLUs, splits and stores its own copy
// of the tile -- the operand stream and the LDS port, not the matrix pipe, bound that loop (tools/x3_abl.sh).  Here the loop
// order is  filter row dy -> K-slice -> dx:  per (dy, K-slice) -- a "group" of three 32-deep steps -- the A stage holds the BM + 2
// plane rows of the flat pixels  m0 + (dy - 1) W - 1 ... m0 + (dy - 1) W + BM,  and step dx reads its A fragments at row offset
// dx (the swizzle key follows the row: one fragment-address set per offset).  9 x BM staged rows per K-slice become 3 x (BM + 2).
//   * rows: output row m and staged pixel p = m + (dy - 1) W + (dx - 1) are FLAT indices, so a staged pixel (b, h', w') is zero
//     unless h' - (dy - 1) is a row of the image (vertical border, batch seam: decided at staging, after the prologue -- BN(0) != 0),
//     and the wrap from one image row into the next cannot be decided there (the same staged row is a valid neighbour of another
//     output): two per-lane predicates, w == 0 and w == W - 1, mask the A fragments of the dx = 0 / dx = 2 steps instead;
//   * the data gradient is the same loop on dy with the taps flipped (weight tap 8 - (3 dy + dx));
//   * pipeline: B is staged per step as there (two register sets, loads two steps ahead of their split).  The A quads of group
//     g + 1 are spread over the three steps of group g (quad k always in the same phase) and written into the other A stage;
//     the load of quad k of group g + 2 is issued right behind: three steps of flight, ONE register set.  One barrier per step.
//   * K splits at group boundaries (launch_igemm_x3 sizes ksteps_per_split in whole groups).
// Epilogue, fix-up, statistics, BatchNorm-backward reduction, prefetch: conv_core.h's, as there.
// ---------------------------------------------------------------------------------------------------------------------
template <int BM, int BN, bool DGRAD, bool PRO, int EPF = 0>
__global__ __launch_bounds__(256) void igemm_x3r_kernel(IgemmArgs a) {
    static_assert(EPF == 0 || (DGRAD && !PRO), "epilogue prefetch: data gradients only");
    constexpr int WGM = 2, WGN = 2, PBK = 32;
    constexpr int RB = BM / WGM / 32, CB = BN / WGN / 32;
    constexpr int RPP = 32;                       // rows per loader pass
    constexpr int AP = BM / RPP, AQ = AP + 1, BP = BN / RPP;      // A quads: AP passes + the two halo rows (quad AP, lanes of rows 0, 1)
    constexpr int ROWB = PBK * 2;
    constexpr int A_PLANE = (BM + 2) * ROWB, B_PLANE = BN * ROWB;
    constexpr int A_STAGE = 3 * A_PLANE, B_STAGE = 3 * B_PLANE, B_BASE = 2 * A_STAGE, OPER = 2 * A_STAGE + 2 * B_STAGE;
    constexpr int NG = PBK / 16;
    static_assert(RB >= 1 && CB >= 1 && AP >= 2 && BP >= 1, "bad tile");
    static_assert(A_STAGE + 2 * A_PLANE + (RB - 1) * 32 * ROWB < 65536 && B_STAGE + 2 * B_PLANE + (CB - 1) * 32 * ROWB < 65536, "fragment offsets are immediates");
    extern __shared__ __attribute__((aligned(16))) float smem[];   // 2 A stages | 2 B stages | BatchNorm block [3][C] (PRO) ; epilogue staging
    char* const lds = reinterpret_cast<char*>(smem);

    DPFT_SETPRIO_IGEMM();
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WGN, wn = wave % WGN;
    int mt, nt, split;
    decode_tile(a, mt, nt, split);
    const int m0 = mt * BM, n0 = nt * BN;

    // ---- loader geometry: quad k < AP stages row rp + 32 k, quad AP rows BM + rp (rp < 2); staged row r of the MIDDLE filter row is pixel m0 - 1 + r
    const int rp = 8 * wave + (lane >> 3);
    const int ch = lane & 7;
    const int hw = a.H * a.W;
    constexpr unsigned OOB = 0x80000000u;
    int a_row[AQ];            // byte offset of that pixel's quad
    unsigned a_mask[AQ];      // bit dy: the pixel one filter row up / the pixel / one down is a row of the same image (bit 3 stays clear)
#pragma unroll
    for (int i = 0; i < AQ; ++i) {
        const int p = m0 - 1 + (i < AP ? rp + RPP * i : BM + rp);
        const bool ok = (i < AP || rp < 2) && p >= 0 && p < a.M;
        const int pp = ok ? p : 0;
        const int h = (pp % hw) / a.W;
        a_row[i] = (pp * a.C + ch * 4) * 4;
        unsigned mask = 0;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) mask |= (ok && (unsigned)(h + dy - 1) < (unsigned)a.H) ? (1u << dy) : 0u;
        a_mask[i] = mask;
    }
    unsigned b_off[BP];
#pragma unroll
    for (int i = 0; i < BP; ++i) {
        const int n = n0 + rp + RPP * i;
        b_off[i] = n < a.N ? (unsigned)(n * a.Ktot + ch * 4) * 4u : OOB;
    }
    const __amdgpu_buffer_rsrc_t rsrc_a =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, a.B * a.H * a.W * a.C * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_b =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, a.N * a.Ktot * 4, 0x00020000);

    const int kt_begin = split * a.ksteps_per_split;      // whole groups (launch_igemm_x3)
    const int kt_end = min(a.ksteps, kt_begin + a.ksteps_per_split);
    const int ngroups = max(kt_end - kt_begin, 0) / 3;
    const int cpt = a.C / PBK;      // groups per filter row
    // group cursors (filter row, channel offset): n1 = the group after the one being consumed (its B tiles are loaded, its A quads
    // split), n2 = the one after that (its A quads are loaded)
    int n1_dy = (kt_begin / 3) / cpt, n1_c0 = (kt_begin / 3 - n1_dy * cpt) * PBK;
    int n2_dy = 0, n2_c0 = 0;
    int la_dy = 3, la_row = 0, la_so = 0;      // A loads: mask bit (3 = the group does not exist), byte offset of the filter row, channel offset
    auto next_group = [&](int& dy, int& c0) {
        c0 += PBK;
        if (c0 == a.C) { c0 = 0; ++dy; }
    };
    auto set_la = [&](int dy, int c0, bool exists) {
        la_dy = exists ? dy : 3;
        la_row = (dy - 1) * a.W * a.C * 4;
        la_so = __builtin_amdgcn_readfirstlane(c0 * 4);
    };
    int so_b = 0;
    auto set_b = [&](int dy, int c0, int dx) {
        const int tap = DGRAD ? 8 - (3 * dy + dx) : 3 * dy + dx;
        so_b = __builtin_amdgcn_readfirstlane((tap * a.C + c0) * 4);
    };

    typedef __attribute__((address_space(3))) const f32x4 lds_f32x4;
    typedef __attribute__((address_space(3))) char lds_char;
    const unsigned lds_base = (unsigned)(size_t)(lds_char*)smem;
    if constexpr (PRO) {
        float* tab = reinterpret_cast<float*>(lds + OPER);
        fill_pro_table(tab, a.pro, a.pro_s, a.C, tid, 256);
    }
    const unsigned ptab_ad = lds_base + OPER + ch * 16;

    // ---- register route ----
    f32x4 rqa[AQ], rqb[2][BP];
    unsigned ra_valid = 0;                         // bit k: A quad k is a real pixel of its filter row (PRO: BN(0) != 0)
    f32x4 p_mu, p_sc, p_sh;
    auto load_a = [&](auto K) {
        constexpr int k = decltype(K)::value;
        const bool v = ((a_mask[k] >> la_dy) & 1u) != 0;
        const unsigned off = v ? (unsigned)(a_row[k] + la_row) : OOB;
        rqa[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_a, (int)off, la_so, 0));
        if constexpr (PRO) ra_valid = (ra_valid & ~(1u << k)) | (v ? (1u << k) : 0u);
    };
    auto load_b = [&](auto SET, auto K) {
        constexpr int set = decltype(SET)::value, k = decltype(K)::value;
        rqb[set][k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_b, (int)b_off[k], so_b, 0));
    };
    const int w_off = rp * ROWB + ((((ch >> 1) ^ ((rp >> 2) & 3)) << 4) | ((ch & 1) << 3));      // (rows BM, BM + 1 carry the key of rows 0, 1)
    auto read_pro = [&](int c0) {
        if constexpr (PRO) {
            const unsigned ad = ptab_ad + (unsigned)c0 * 4u;
            p_mu = *(lds_f32x4*)(size_t)(ad);
            p_sc = *(lds_f32x4*)(size_t)(ad + (unsigned)a.C * 4u);
            p_sh = *(lds_f32x4*)(size_t)(ad + (unsigned)a.C * 8u);
        }
    };
    // pieces of a quad's way into LDS, as in igemm_x3_kernel: 0, 1 BN + ReLU | 2 padding mask | 3..6 split | 7 LDS writes
    // (A quads with prologue: 0..7, all others 3..7).  A quad k goes to A stage AST, B quad k from register set / to B stage BST.
    f32x4 cv;
    u32x2 c1, c2, c3;
    float rr0 = 0.f, rr1 = 0.f;
    auto piece = [&](auto ISA_, auto ST_, auto K, auto ID) __attribute__((always_inline)) {
        constexpr bool isa = decltype(ISA_)::value;
        constexpr int st = decltype(ST_)::value, k = decltype(K)::value, id = decltype(ID)::value;
        constexpr bool bn = PRO && isa;
        if constexpr (id == 0 || id == 1) {
            static_assert(bn, "BatchNorm pieces: A quads of a PRO kernel");
            if constexpr (id == 0) cv = rqa[k];
#pragma unroll
            for (int e = 2 * id; e < 2 * id + 2; ++e) cv[e] = fmaxf(fmaf(cv[e] - p_mu[e], p_sc[e], p_sh[e]), 0.f);
        } else if constexpr (id == 2) {
            const unsigned keep = (unsigned)__builtin_amdgcn_sbfe(ra_valid, k, 1);
#pragma unroll
            for (int e = 0; e < 4; ++e) cv[e] = __uint_as_float(__float_as_uint(cv[e]) & keep);
        } else if constexpr (id == 3 || id == 5) {
            constexpr int h = (id - 3) / 2;
            if constexpr (id == 3 && !bn) {
                if constexpr (isa) cv = rqa[k];
                else cv = rqb[st][k];
            }
            const float x = cv[2 * h], y = cv[2 * h + 1];
            const unsigned q = cvt_pk_bf16(x, y);
            c1[h] = q;
            rr0 = x - __uint_as_float(q << 16);
            rr1 = y - __uint_as_float(q & 0xffff0000u);
        } else if constexpr (id == 4 || id == 6) {
            constexpr int h = (id - 4) / 2;
            const unsigned q = cvt_pk_bf16(rr0, rr1);
            c2[h] = q;
            c3[h] = cvt_pk_bf16(rr0 - __uint_as_float(q << 16), rr1 - __uint_as_float(q & 0xffff0000u));
        } else {
            constexpr int PL = isa ? A_PLANE : B_PLANE;
            char* dst = lds + (isa ? st * A_STAGE + (k < AP ? k * RPP : BM) * ROWB : B_BASE + st * B_STAGE + k * RPP * ROWB) + w_off;
            if (!isa || k < AP || rp < 2) {
                *reinterpret_cast<u32x2*>(dst) = c1;
                *reinterpret_cast<u32x2*>(dst + PL) = c2;
                *reinterpret_cast<u32x2*>(dst + 2 * PL) = c3;
            }
        }
    };
    constexpr int NPA = PRO ? 8 : 5, NPB = 5;

    f32x16 acc[RB][CB], acl[RB][CB];
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
        for (int j = 0; j < CB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[i][j][r] = 0.f; acl[i][j][r] = 0.f; }

    // ---- epilogue-operand prefetch (as igemm_x3_kernel) ----
    constexpr int EP_ITER = BM * (BN / 4) / 256;
    using PFT = EpiPrefetch<EP_ITER, false, EPF>;
    PFT pf;
    auto pf_op = [&](auto IT_, auto KIND_) __attribute__((always_inline)) {
        if constexpr (EPF != 0) {
            constexpr int it = decltype(IT_)::value, kind = decltype(KIND_)::value;
            constexpr int C4 = BN / 4;
            int t = tid;
            asm volatile("" : "+v"(t));
            const int idx = t + it * 256;
            const int row = idx / C4, c4 = idx - row * C4;
            const bool ok = m0 + row < a.M && n0 + c4 * 4 < a.N;
            const unsigned el = ok ? (unsigned)(m0 + row) * (unsigned)a.N + (unsigned)(n0 + c4 * 4)
                                   : (unsigned)m0 * (unsigned)a.N + (unsigned)n0;
            using Q = typename PFT::Q;
            if constexpr (kind == 0) pf.y[it] = *reinterpret_cast<const Q*>(reinterpret_cast<const char*>(a.bnr_y) + (size_t)el * 4);
            else if constexpr (kind == 1) { if constexpr (EPF == 1) pf.g[it] = *reinterpret_cast<const Q*>(reinterpret_cast<const char*>(a.res_src) + (size_t)el * 4); }
            else if constexpr (kind == 2) { if (EPF == 1 || a.bnr_mask8) pf.mk[it] = a.bnr_mask8[el >> 2]; }
            else { if constexpr (EPF == 1) pf.rm[it] = a.res_mask8[el >> 2]; }
        }
    };

    // ---- fragment addresses: lane l reads staged row l % 32 + dx of a 32-row block; stage, plane and block offsets are immediates ----
    const int hh = lane >> 5;
    unsigned a_ad[NG][3], b_ad[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int row = (lane & 31) + dx;
            a_ad[g][dx] = lds_base + (wm * RB * 32 + row) * ROWB + (((2 * g + hh) ^ ((row >> 2) & 3)) << 4);
            asm volatile("" : "+v"(a_ad[g][dx]));
        }
        b_ad[g] = lds_base + B_BASE + (wn * CB * 32 + (lane & 31)) * ROWB + (((2 * g + hh) ^ (((lane & 31) >> 2) & 3)) << 4);
        asm volatile("" : "+v"(b_ad[g]));
    }
    // the wrap predicates of this lane's output rows: keep[0] clears the dx = 0 fragments where w == 0, keep[1] the dx = 2 ones where w == W - 1
    unsigned keep[2][RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        const int w = (m0 + (wm * RB + i) * 32 + (lane & 31)) % a.W;
        keep[0][i] = w == 0 ? 0u : ~0u;
        keep[1][i] = w == a.W - 1 ? 0u : ~0u;
    }

    // One step: consumes B stage STG and A stage AST at row offset PH.  Unless FIN (the split's last group): splits this phase's A
    // quads of the next group into the other A stage and loads the same quads of the group after it; splits B tile t + 1 (register
    // set / stage STG ^ 1) and loads tile t + 3 into that set.  FIN: the B tiles left in the group, no loads.
    constexpr int MPG = 6 * RB * CB, SLOTS = NG * MPG;
    constexpr int NRD = 3 * (RB + CB);      // fragment reads per K-group, in the order of first use (MFMA terms: a3 b1, a2 b1, a1 b1, a2 b2, a1 b2, a1 b3)
    auto step = [&](auto STG_, auto AST_, auto PH_, auto FIN_) __attribute__((always_inline)) {
        constexpr int stg = decltype(STG_)::value, ast = decltype(AST_)::value, ph = decltype(PH_)::value;
        constexpr bool fin = decltype(FIN_)::value;
        constexpr bool m1 = !(fin && ph == 2), m2 = !fin;
        constexpr int ka0 = fin ? 0 : ph * AQ / 3, ka1 = fin ? 0 : (ph + 1) * AQ / 3;
        constexpr int NPCA = (ka1 - ka0) * NPA, NPC = NPCA + (m1 ? BP * NPB : 0);
        using OTHER = std::integral_constant<int, (stg ^ 1)>;
        using AOTHER = std::integral_constant<int, (ast ^ 1)>;
        if constexpr (m2) set_b(n1_dy, n1_c0, ph);
        if constexpr (!fin) read_pro(n1_c0);
        bf16x8 af[2][3][RB], bf[2][3][CB];
        auto frag_one = [&](auto SET, auto G, auto R) {      // read R: A plane 2 | B plane 0 | A plane 1 | A plane 0 | B plane 1 | B plane 2
            constexpr int set = decltype(SET)::value, g = decltype(G)::value, r = decltype(R)::value;
            constexpr bool isa = r < RB || (r >= RB + CB && r < 3 * RB + CB);
            if constexpr (isa) {
                constexpr int p = r < RB ? 2 : (r < 2 * RB + CB ? 1 : 0), o = r < RB ? r : (r - RB - CB) % RB;
                af[set][p][o] = __builtin_bit_cast(bf16x8, *(lds_f32x4*)(size_t)(a_ad[g][ph] + (unsigned)(ast * A_STAGE + p * A_PLANE + o * 32 * ROWB)));
            } else {
                constexpr int p = r < RB + CB ? 0 : 1 + (r - 3 * RB - CB) / CB, o = r < RB + CB ? r - RB : (r - 3 * RB - CB) % CB;
                bf[set][p][o] = __builtin_bit_cast(bf16x8, *(lds_f32x4*)(size_t)(b_ad[g] + (unsigned)(stg * B_STAGE + p * B_PLANE + o * 32 * ROWB)));
            }
        };
        // The wrap mask of a dx = 0 / dx = 2 step: rows whose neighbour lies in another image row leave the product.  Each A fragment
        // (plane p, block i) is masked in the MFMA slot before its first use -- slot (2 - p) RB CB + i CB of its K-group -- so that no
        // mask waits for an LDS read the matrix pipe does not wait for yet; USE = -1: those of slot 0, masked in the slot before the group.
        auto wrap_at = [&](auto SET, auto USE_) {
            constexpr int set = decltype(SET)::value, use = decltype(USE_)::value;
            if constexpr (ph != 1) {
                static_for<3 * RB>([&](auto Q) {
                    constexpr int p = decltype(Q)::value / RB, o = decltype(Q)::value % RB;
                    if constexpr ((2 - p) * RB * CB + o * CB - 1 == use) {
                        u32x4 v = __builtin_bit_cast(u32x4, af[set][p][o]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] &= keep[ph / 2][o];
                        af[set][p][o] = __builtin_bit_cast(bf16x8, v);
                    }
                });
            }
        };
        static_for<NRD>([&](auto R) { frag_one(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, R); });
        wrap_at(std::integral_constant<int, 0>{}, std::integral_constant<int, -1>{});
        __builtin_amdgcn_sched_barrier(0);
        static_for<SLOTS>([&](auto S) {
            constexpr int sl = decltype(S)::value;
            constexpr int g = sl / MPG, w = sl % MPG, t = w / (RB * CB), ij = w % (RB * CB), i = ij / CB, j = ij % CB;
            constexpr int TA[6] = {2, 1, 0, 1, 0, 0}, TB[6] = {0, 0, 0, 1, 1, 2};
            if constexpr (t == 2)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[g & 1][0][i], bf[g & 1][0][j], acc[i][j], 0, 0, 0);
            else
                acl[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[g & 1][TA[t]][i], bf[g & 1][TB[t]][j], acl[i][j], 0, 0, 0);
            if constexpr (g + 1 < NG) {
                constexpr int r0 = w * NRD / MPG, r1 = (w + 1) * NRD / MPG;
                static_for<r1 - r0>([&](auto R) {
                    frag_one(std::integral_constant<int, ((g + 1) & 1)>{}, std::integral_constant<int, (g + 1 < NG ? g + 1 : 0)>{},
                             std::integral_constant<int, r0 + decltype(R)::value>{});
                });
                if constexpr (w == MPG - 1) wrap_at(std::integral_constant<int, ((g + 1) & 1)>{}, std::integral_constant<int, -1>{});
            }
            wrap_at(std::integral_constant<int, (g & 1)>{}, std::integral_constant<int, w>{});
            if constexpr (NPC > 0) {
                constexpr int p0 = sl * NPC / SLOTS, p1 = (sl + 1) * NPC / SLOTS;
                static_for<p1 - p0>([&](auto Q) {
                    constexpr int P = p0 + decltype(Q)::value;
                    if constexpr (P < NPCA) {
                        constexpr int k = ka0 + P / NPA, o = P % NPA;
                        piece(std::true_type{}, AOTHER{}, std::integral_constant<int, k>{}, std::integral_constant<int, (PRO ? o : o + 3)>{});
                        if constexpr (o == NPA - 1) load_a(std::integral_constant<int, k>{});
                    } else {
                        constexpr int k = (P - NPCA) / NPB, o = (P - NPCA) % NPB;
                        piece(std::false_type{}, OTHER{}, std::integral_constant<int, k>{}, std::integral_constant<int, o + 3>{});
                        if constexpr (m2 && o == NPB - 1) load_b(OTHER{}, std::integral_constant<int, k>{});
                    }
                });
            }
            __builtin_amdgcn_sched_barrier(0);
        });
    };
    auto fence = [&]() {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, 1>;
    using S2 = std::integral_constant<int, 2>;
    using T = std::true_type;
    using F = std::false_type;

    if constexpr (PRO) __syncthreads();      // the BatchNorm table is in LDS
    if (ngroups > 0) {      // group 0 -> A stage 0, its first B tile -> B stage 0; then A of group 1, B tiles 1, 2 of group 0 -> the registers
        set_la(n1_dy, n1_c0, true);
        set_b(n1_dy, n1_c0, 0);
        static_for<AQ>([&](auto K) { load_a(K); });
        static_for<BP>([&](auto K) { load_b(S0{}, K); });
        read_pro(n1_c0);
        static_for<AQ * NPA>([&](auto P_) {
            constexpr int P = decltype(P_)::value, o = P % NPA;
            piece(T{}, S0{}, std::integral_constant<int, P / NPA>{}, std::integral_constant<int, (PRO ? o : o + 3)>{});
        });
        static_for<BP * NPB>([&](auto P_) {
            constexpr int P = decltype(P_)::value;
            piece(F{}, S0{}, std::integral_constant<int, P / NPB>{}, std::integral_constant<int, P % NPB + 3>{});
        });
        set_b(n1_dy, n1_c0, 1);
        static_for<BP>([&](auto K) { load_b(S1{}, K); });
        set_b(n1_dy, n1_c0, 2);
        static_for<BP>([&](auto K) { load_b(S0{}, K); });
        next_group(n1_dy, n1_c0);
        set_la(n1_dy, n1_c0, ngroups > 1);
        static_for<AQ>([&](auto K) { load_a(K); });
        n2_dy = n1_dy; n2_c0 = n1_c0;
        next_group(n2_dy, n2_c0);
        set_la(n2_dy, n2_c0, ngroups > 2);
    }
    if constexpr (EPF != 0) {
        static_for<EP_ITER * 4>([&](auto O) {
            constexpr int o = decltype(O)::value;
            pf_op(std::integral_constant<int, o / 4>{}, std::integral_constant<int, o % 4>{});
        });
    }
    fence();
    // a group = three steps; two groups bring every stage and register set back to where it was.  The loop body is branch-free
    // (a branch inside it makes the compiler carry accumulators and in-flight loads through copies at the loop's end)
    int done = 0;      // groups consumed
    auto group_end = [&]() {
        ++done;
        n1_dy = n2_dy; n1_c0 = n2_c0;
        next_group(n2_dy, n2_c0);
        set_la(n2_dy, n2_c0, done + 2 < ngroups);
    };
    auto half0 = [&](auto FIN_) __attribute__((always_inline)) {
        step(S0{}, S0{}, S0{}, FIN_); fence(); step(S1{}, S0{}, S1{}, FIN_); fence(); step(S0{}, S0{}, S2{}, FIN_);
    };
    auto half1 = [&](auto FIN_) __attribute__((always_inline)) {
        step(S1{}, S1{}, S0{}, FIN_); fence(); step(S0{}, S1{}, S1{}, FIN_); fence(); step(S1{}, S1{}, S2{}, FIN_);
    };
    int rem = ngroups;
    for (; rem > 2; rem -= 2) {
        half0(F{}); fence(); group_end();
        half1(F{}); fence(); group_end();
    }
    if (rem == 2) {
        half0(F{}); fence(); group_end();
        half1(T{});
    } else if (rem == 1) {
        half0(T{});
    }
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
        for (int j = 0; j < CB; ++j) acc[i][j] += acl[i][j];
    if constexpr (EPF != 0) igemm_epilogue<BM, BN, WGM, WGN, RB, CB, 256, PFT>(a, acc, m0, n0, mt, split, smem, &pf);
    else igemm_epilogue<BM, BN, WGM, WGN, RB, CB, 256>(a, acc, m0, n0, mt, split, smem);
}


template <typename K>
static void launch_x3r(K kernel, dim3 grid, size_t lds, hipStream_t st, const IgemmArgs& args) {
    static LdsGrant grant;      // one per kernel instantiation
    (void)lds_grant(grant, reinterpret_cast<const void*>(kernel), lds);
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, args);
}

// One tile's instantiations.  The prefetching data gradients exist below 128 x 128 only, as in launch_igemm_x3 (at 128 x 128 the
// prefetched operands do not fit the register file).
template <int BM, int BN>
static void launch_x3r_tile(const IgemmArgs& a, bool dgrad, bool pro, dim3 grid, size_t lds, hipStream_t st) {
    if (!dgrad) {
        if (pro) launch_x3r(igemm_x3r_kernel<BM, BN, false, true, 0>, grid, lds, st, a);
        else launch_x3r(igemm_x3r_kernel<BM, BN, false, false, 0>, grid, lds, st, a);
        return;
    }
    if constexpr (BM * BN < 128 * 128) {
        if (a.epf == 1) { launch_x3r(igemm_x3r_kernel<BM, BN, true, false, 1>, grid, lds, st, a); return; }
        if (a.epf == 2) { launch_x3r(igemm_x3r_kernel<BM, BN, true, false, 2>, grid, lds, st, a); return; }
    }
    launch_x3r(igemm_x3r_kernel<BM, BN, true, false, 0>, grid, lds, st, a);
}

int launch_igemm_x3r(IgemmArgs& a, int bm, int bn, bool dgrad, bool pro, hipStream_t st) {
    DPFT_REQUIRE(!(a.x3 && a.w3) && a.kh == 3 && a.kw == 3 && a.stride == 1 && a.pad == 1 && a.sub_step <= 1 && a.C % 32 == 0 &&
                     a.ksteps == 9 * (a.C / 32) && a.H == a.OH && a.W == a.OW && !(dgrad && pro),
                 "conv x3 row-shared form: 3x3, stride 1, pad 1, C %% 32 == 0");
    a.ksteps_per_split = 3 * cdiv(a.ksteps / 3, a.splits);      // the K split falls between (filter row, K-slice) groups
    const dim3 grid(a.mtiles * a.ntiles * a.splits);
    const size_t lds = std::max((size_t)2 * 3 * (bm + 2 + bn) * 64 + (pro ? (size_t)12 * a.C : 0), (size_t)bm * (bn + 4) * 4 + (size_t)3 * bn * 4);
    if (bm == 128 && bn == 128) launch_x3r_tile<128, 128>(a, dgrad, pro, grid, lds, st);
    else if (bm == 128 && bn == 64) launch_x3r_tile<128, 64>(a, dgrad, pro, grid, lds, st);
    else launch_x3r_tile<64, 64>(a, dgrad, pro, grid, lds, st);
    return check_launch("conv igemm (3 x bf16 split, row-shared)");
}

}  // namespace dpft
