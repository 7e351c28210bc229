// Rotated-box NMS between the model and its consumers (dpft_amd/evaluation/nms.py holds the definition; tests/nms_ref.py restates
// it in numpy fp64).  The reference has no such step.  Per batch, three launches on the caller's stream, no host read-back:
//   sort pass   one workgroup per frame: argmax class and score of every query (the rule of ap_argmax), cls copied to cls_out bit
//               for bit, statuses -2 (no candidate) / -3 (below min_score); the candidates are compacted and sorted in LDS by
//               (score desc, query asc) -- the key of ap_match_kernel -- and written to scratch in that order: query, class, score
//               and the 8 box floats.
//   mask pass   one lane per ordered pair (i, j), i < j in sorted order; a wave covers 64 consecutive j of one i, so the ballot of
//               "IoU > threshold" IS the 64-bit word (i, j / 64) of the suppression matrix.  fp64 end to end (box_iou.h; this file
//               is built with -ffp-contract=off): the strict comparison decides exactly as the fp64 restatement does.  Pairs of
//               different classes are skipped (unless class-agnostic), and so are pairs whose circumscribed circles are apart
//               by a margin: their clip is empty, the IoU exactly 0 <= threshold -- the reject never changes a decision.
//   scan pass   one wave per frame walks the candidates in blocks of 64.  Lane m owns the "removed" word of block m.  Within a
//               block the 64 diagonal words are lane-private and the kept rows are visited in order (a cross-lane read per kept
//               row); then the kept rows' words of every later block are OR-reduced over the wave into that block's removed word,
//               and only the newly removed candidates look for their first suppressor.  Writes status, order, counts and the
//               [n, 0] entries of cls_out.
// Nothing is accumulated in floating point and nothing depends on the order in which workgroups run: the same input gives the
// same bits.
#include "common.h"
#include "box_iou.h"
#include "nms_layout.h"

#include <limits.h>
#include <math.h>

namespace dpft {

constexpr int kNmsMaxN = 1024, kNmsMaxC = 16, kNmsMaxW = kNmsMaxN / 64;

struct NmsArgs {
    const float *cls, *center, *size, *angle;      // (B,N,C) (B,N,3) (B,N,3) (B,N,2)
    // scratch, all in sorted order per frame: only the first ndet[b] entries of a frame are written and read
    unsigned long long* mask;                      // (B, W, W, 64): word [i / 64][w][i % 64] = bits j = 64 w .. 64 w + 63 of row i
    float* box;                                    // (B,N,8)
    int* label;                                    // (B,N)
    int* sorted;                                   // (B,N) query index
    float* score;                                  // (B,N)
    int* ndet;                                     // (B)
    int32_t *status, *order, *counts;              // (B,N) (B,N) (B)
    float* cls_out;                                // (B,N,C)
    double thr;
    float min_score;
    int kind, agnostic, max_det;
    int B, N, C, W;                                // W = ceil(N / 64)
};

__global__ __launch_bounds__(256) void nms_sort_kernel(NmsArgs a) {
    __shared__ unsigned long long key[kNmsMaxN];      // (score descending, query ascending) as one ascending integer
    __shared__ float score[kNmsMaxN];
    __shared__ unsigned char label[kNmsMaxN];
    __shared__ int s_D;
    const int b = blockIdx.x, tid = threadIdx.x, N = a.N, C = a.C;
    if (tid == 0) s_D = 0;
    __syncthreads();
    // ---- candidates of the frame (compacted in arrival order: the sort below fixes the order) ----
    for (int n = tid; n < N; n += 256) {
        const int64_t r = (int64_t)b * N + n;
        const float* row = a.cls + r * C;
        float s;
        const int l = ap_argmax(row, C, s);
        const unsigned* src = (const unsigned*)row;
        unsigned* dst = (unsigned*)(a.cls_out + r * C);
        for (int k = 0; k < C; ++k) dst[k] = src[k];
        label[n] = (unsigned char)l;
        score[n] = s;
        int st = -2;
        if (l != 0 && s == s) {
            if (!(s >= a.min_score)) {
                st = -3;
                a.cls_out[r * C] = s;
            } else {
                st = -1;                                                    // (the scan pass decides)
                unsigned u = __float_as_uint(s);
                if (u == 0x80000000u) u = 0u;                               // -0 orders as +0
                const unsigned ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
                key[atomicAdd(&s_D, 1)] = ((unsigned long long)(~ord) << 32) | (unsigned)n;
            }
        }
        a.status[r] = st;
        a.order[r] = -1;
    }
    __syncthreads();
    const int D = s_D;
    int P = 1;
    while (P < D) P <<= 1;
    for (int i = D + tid; i < P; i += 256) key[i] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {                                      // bitonic sort, ascending
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += 256) {
                const int x = i ^ j;
                if (x > i) {
                    const unsigned long long u = key[i], v = key[x];
                    if ((u > v) == ((i & k) == 0)) { key[i] = v; key[x] = u; }
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < D; i += 256) {
        const int q = (int)(unsigned)key[i];
        const int64_t r = (int64_t)b * N + q, o = (int64_t)b * N + i;
        const float *ce = a.center + r * 3, *sz = a.size + r * 3, *an = a.angle + r * 2;
        float4* bx = (float4*)(a.box + o * 8);
        bx[0] = make_float4(ce[0], ce[1], ce[2], sz[0]);
        bx[1] = make_float4(sz[1], sz[2], an[0], an[1]);
        a.sorted[o] = q;
        a.label[o] = label[q];
        a.score[o] = score[q];
    }
    if (tid == 0) a.ndet[b] = D;
}

// true only where the IoU of the pair is 0 by the definition or certainly 0 by the geometry (never above a threshold inside (0, 1)):
//  * one of the 16 numbers is not finite: the definition gives such a box IoU 0 with everything (where x, y, l, w, sin or cos is not
//    finite no comparison of the clip holds anyway; z and h are named so that fmin / fmax skipping a NaN cannot matter);
//  * the circumscribed circles of the two footprints apart by more than 0.1 % + 1 mm: the clip comes out empty.
__device__ __forceinline__ bool nms_certainly_zero(const float* p, const float* q) {
    float fin = 0.0f;
    for (int k = 0; k < 8; ++k) fin += (p[k] - p[k]) + (q[k] - q[k]);      // (x - x is NaN for x = NaN, +-inf)
    if (!(fin == 0.0f)) return true;
    const double dx = (double)q[0] - (double)p[0], dy = (double)q[1] - (double)p[1];
    const double R = (hypot((double)p[3], (double)p[4]) + hypot((double)q[3], (double)q[4])) / 2;
    const double lim = R * 1.001 + 1e-3;
    return dx * dx + dy * dy > lim * lim;
}

__global__ __launch_bounds__(256) void nms_mask_kernel(NmsArgs a) {
    const int lane = threadIdx.x & 63, W = a.W, N = a.N;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);        // one wave per (frame, row i, word w)
    const int64_t per = (int64_t)N * W;
    if (g >= (int64_t)a.B * per) return;
    const int b = (int)(g / per);
    const int r = (int)(g % per);
    const int i = r / W, w = r % W;
    const int D = a.ndet[b];
    if (i >= D || w < (i >> 6) || w * 64 >= D) return;                      // (uniform over the wave; the scan reads no other word)
    const int j = w * 64 + lane;
    bool bit = false;
    if (j > i && j < D) {
        const int64_t oi = (int64_t)b * N + i, oj = (int64_t)b * N + j;
        if (a.agnostic || a.label[oi] == a.label[oj]) {
            float p[8], q[8];
            const float4 *pi = (const float4*)(a.box + oi * 8), *pj = (const float4*)(a.box + oj * 8);
            const float4 p0 = pi[0], p1 = pi[1], q0 = pj[0], q1 = pj[1];
            p[0] = p0.x; p[1] = p0.y; p[2] = p0.z; p[3] = p0.w; p[4] = p1.x; p[5] = p1.y; p[6] = p1.z; p[7] = p1.w;
            q[0] = q0.x; q[1] = q0.y; q[2] = q0.z; q[3] = q0.w; q[4] = q1.x; q[5] = q1.y; q[6] = q1.z; q[7] = q1.w;
            if (!nms_certainly_zero(p, q)) {
                double bev, d3;
                ap_iou_pair(p, p + 3, p + 6, q, q + 3, q + 6, bev, d3);     // box 1 = the earlier candidate
                bit = (a.kind ? d3 : bev) > a.thr;
            }
        }
    }
    const unsigned long long word = __ballot(bit);
    if (lane == 0) a.mask[(((int64_t)b * W + (i >> 6)) * W + w) * 64 + (i & 63)] = word;
}

__device__ __forceinline__ unsigned long long nms_wave_or(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}

// the 64-bit value of one lane, `lane` wave-uniform: two v_readlane instead of a trip through the LDS crossbar
__device__ __forceinline__ unsigned long long nms_readlane(unsigned long long v, int lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}

// every loop below runs on wave-uniform conditions: all 64 lanes stay active through the cross-lane reads
__global__ __launch_bounds__(64) void nms_scan_kernel(NmsArgs a) {
    __shared__ int sup[kNmsMaxN];      // first suppressor (sorted index) or -1; entry 64 m + lane is only ever touched by `lane`
    const int b = blockIdx.x, lane = threadIdx.x, N = a.N, W = a.W, C = a.C;
    const int D = a.ndet[b];
    const int nb = (D + 63) >> 6;
    const unsigned long long* mask = a.mask + (int64_t)b * W * W * 64;
    const int64_t base = (int64_t)b * N;
    unsigned long long removed = 0ull;                                      // lane m: the candidates of block m suppressed so far
    for (int m = 0; m < nb; ++m) sup[64 * m + lane] = -1;
    int kept_before = 0;
    for (int k = 0; k < nb; ++k) {
        const int i = 64 * k + lane;
        const bool valid = i < D;
        const unsigned long long vmask = __ballot(valid);
        const unsigned long long* rowp = mask + (int64_t)k * W * 64 + lane;
        const unsigned long long diag = valid ? rowp[(int64_t)k * 64] : 0ull;
        unsigned long long later[kNmsMaxW];                                 // this row's words of the later blocks, all loads in flight at once
#pragma unroll
        for (int m = 0; m < kNmsMaxW; ++m) later[m] = (valid && m > k && m < nb) ? rowp[(int64_t)m * 64] : 0ull;
        // ---- the diagonal: kept rows in order; a row's word only has bits above its own ----
        unsigned long long rem = nms_readlane(removed, __builtin_amdgcn_readfirstlane(k));
        int mysup = sup[i];
        unsigned long long todo = vmask & ~rem;
        while (todo) {
            const int t = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);      // the next kept row
            const unsigned long long row = nms_readlane(diag, t);
            if (((row & ~rem) >> lane) & 1ull) mysup = 64 * k + t;
            rem |= row;
            todo &= ~(rem | (1ull << t));
        }
        const unsigned long long kept = vmask & ~rem;
        const bool me_kept = (kept >> lane) & 1ull;
        // ---- the kept rows' words into the later blocks; only newly removed candidates look for their (first) suppressor ----
#pragma unroll
        for (int m = 0; m < kNmsMaxW; ++m) {
            if (m > k && m < nb) {
                const unsigned long long mine = me_kept ? later[m] : 0ull;
                if (__ballot(mine != 0ull) == 0ull) continue;               // (most block pairs: no kept row reaches block m)
                const unsigned long long any = nms_wave_or(mine);
                unsigned long long fresh = any & ~nms_readlane(removed, m);
                if (fresh) {
                    int s = sup[64 * m + lane];
                    unsigned long long rows = __ballot((mine & fresh) != 0ull);
                    while (rows) {
                        const int t = __builtin_amdgcn_readfirstlane(__ffsll((long long)rows) - 1);
                        const unsigned long long wt = nms_readlane(mine, t);
                        if (((wt & fresh) >> lane) & 1ull) s = 64 * k + t;
                        fresh &= ~wt;
                        rows = __ballot((mine & fresh) != 0ull);
                    }
                    sup[64 * m + lane] = s;
                    if (lane == m) removed |= any;
                }
            }
        }
        // ---- block k is final ----
        if (valid) {
            const int q = a.sorted[base + i];
            const int rank = kept_before + __popcll(kept & ((1ull << lane) - 1ull));
            int st;
            if (!me_kept) st = a.sorted[base + mysup];
            else if (rank >= a.max_det) st = -4;
            else { st = -1; a.order[base + rank] = q; }
            a.status[base + q] = st;
            if (st != -1) a.cls_out[(base + q) * C] = a.score[base + i];
        }
        kept_before += __popcll(kept);
    }
    if (lane == 0) a.counts[b] = min(kept_before, a.max_det);
}

}  // namespace dpft

using namespace dpft;

extern "C" int64_t dpft_nms_scratch_bytes(int32_t B, int32_t N) {
    if (!(B >= 0 && B <= 65536 && N >= 0 && N <= kNmsMaxN)) {
        set_error("nms_scratch_bytes: sizes out of range (0 <= B <= 65536, 0 <= N <= %d)", kNmsMaxN);
        return -1;
    }
    if (B == 0 || N == 0) return 0;
    // mask, then box (8 floats), label, sorted, score per query, then the candidate count per frame (nms_layout.h)
    return nms_scratch_size(B, N);
}

extern "C" int dpft_nms_f32(const float* cls, const float* center, const float* size, const float* angle, const double* iou,
                            int32_t kind, int32_t class_agnostic, float min_score, int32_t max_det, void* scratch,
                            int32_t* status, int32_t* order, int32_t* counts, float* cls_out, int32_t B, int32_t N, int32_t C,
                            dpft_stream_t stream) {
    DPFT_REQUIRE(B >= 0 && B <= 65536 && N >= 0 && N <= kNmsMaxN && C >= 2 && C <= kNmsMaxC,
                 "nms: sizes out of range (0 <= B <= 65536, 0 <= N <= %d, 2 <= C <= %d), got B %d, N %d, C %d", kNmsMaxN, kNmsMaxC,
                 B, N, C);
    DPFT_REQUIRE(iou, "nms: null argument (iou)");
    DPFT_REQUIRE(*iou > 0.0 && *iou < 1.0, "nms: the IoU threshold must lie inside (0, 1), got %g", *iou);
    DPFT_REQUIRE(kind == 0 || kind == 1, "nms: kind 0 (bev) or 1 (3d), got %d", kind);
    DPFT_REQUIRE(min_score == min_score, "nms: min_score is NaN (-INFINITY = no filter)");
    DPFT_REQUIRE(max_det >= 1, "nms: max_det must be >= 1 (INT32_MAX = no limit), got %d", max_det);
    if (B == 0 || N == 0) return DPFT_OK;
    DPFT_REQUIRE(cls && center && size && angle && scratch && status && order && counts && cls_out, "nms: null argument");
    DPFT_REQUIRE(cls_out != cls, "nms: cls_out must not alias cls");
    DPFT_REQUIRE(((uintptr_t)scratch & 15) == 0, "nms: scratch needs 16-byte alignment");
    NmsArgs a;
    memset(&a, 0, sizeof(a));
    const int W = (N + 63) / 64;
    const NmsScratch sc = nms_scratch_layout(scratch, B, N);
    a.mask = sc.mask; a.box = sc.box; a.label = sc.label; a.sorted = sc.sorted; a.score = sc.score; a.ndet = sc.ndet;
    a.cls = cls; a.center = center; a.size = size; a.angle = angle;
    a.status = status; a.order = order; a.counts = counts; a.cls_out = cls_out;
    a.thr = *iou; a.min_score = min_score; a.kind = kind; a.agnostic = class_agnostic != 0; a.max_det = max_det;
    a.B = B; a.N = N; a.C = C; a.W = W;
    hipLaunchKernelGGL(nms_sort_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
    int rc = check_launch("nms sort");
    if (rc) return rc;
    const int64_t waves = (int64_t)B * N * W;
    hipLaunchKernelGGL(nms_mask_kernel, dim3((unsigned)cdiv(waves, 4)), dim3(256), 0, (hipStream_t)stream, a);
    rc = check_launch("nms mask");
    if (rc) return rc;
    hipLaunchKernelGGL(nms_scan_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
    return check_launch("nms scan");
}
