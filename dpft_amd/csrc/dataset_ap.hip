// Split-level AP_BEV / AP_3D accumulated on the device during evaluation (dpft_amd/evaluation/dataset_ap.py holds the
// definition; tests/dataset_ap_ref.py restates it in numpy fp64).
//
// update, per batch, two launches, no host read-back:
//   pair pass   one thread per (sample, query, target): BEV and 3D IoU in fp64 into a (B,N,Mmax,2) scratch.  fp64 end to end (this
//               file is built with -ffp-contract=off): the strict "IoU > threshold" rule then decides exactly as the fp64 restatement
//               does, also where an IoU equals a threshold exactly.
//   match pass  one workgroup per sample: detections compacted and sorted in LDS by (score desc, query asc), then one wave per
//               (IoU kind, threshold) combination walks them in order; the lanes hold the targets (<= 4 per lane, the "assigned"
//               bits are lane-private registers), a wave reduction picks the best unassigned target above the threshold.  The
//               workgroup reserves its records with ONE integer atomic on a device cursor and appends 16-byte records.
// finalize, once per epoch: one workgroup per (class, combination) scans that class's ordered records (block prefix sum of the TP
//               bits) into R recall bins (64-bit integer max of the precision's bit pattern), suffix maximum, AP.
// The clip (box_iou.h, shared with nms.hip) takes (sin, cos) directly -- no atan2.
//
// Scene-description groups (optional, the *_groups entries): the match pass's workgroup also writes one row of a frame store
// (frame, group bitmask from the frame's [road, time, weather] description, npos per class) at a host-known position -- no atomic;
// the grouped finalize sums the frame rows per group (integers) and scans one workgroup per (group, class, combination) with two
// block prefix sums per trip, membership and member-and-TP: the rank inside the group is the membership prefix.  Bin rule, suffix
// maximum and summation order are ap_finalize_kernel's, so a group's table has the bits of an ungrouped run over its frames.
//
// True-positive errors (optional, the *_tp entries): the wave of the match pass that owns the reference combination keeps the target
// index it took per sorted detection in LDS; the append loop turns every TP of that combination into four fp64 errors (centre
// distance, height, size, heading) and writes them as int64 fixed point (rint(e * 2^32)) into a second store at the record's
// position, zeros for every other record.  Integer sums are exact and order-free, so the finalize (one workgroup per class, or per
// (group, class): block scan of the TP bit and of the four integers, cumulative means at the recall points) gives a group the bits
// of an ungrouped run over its frames, and a merge of ranks cannot move a bit.
//
// KITTI-protocol table (optional, the *_kitti entries; the protocol and its two reductions are stated in
// dpft_amd/evaluation/dataset_ap.py, tests/dataset_ap_kitti_ref.py holds the literal two passes).  After the walk above the wave
// that owns a combination walks twice more: pass 1 (target-major, every target takes the first unassigned detection in score
// order above the threshold) sets bit 8 + k of the record's fourth word, pass 2 (the detections inserted in score order into a
// maintained target-major largest-IoU matching, a displaced detection offered on to the later targets) sets bit 16 + k when the
// insertion adds a matched target.  Over the split's ordered records the protocol is then two prefix sums: the pass-1 bits rank
// the TP scores the <= 41 thresholds are picked from (ap_kitti.h), the pass-2 bits up to the end of a threshold's score tie group
// are its TP count.  The one-bit form of pass 2 holds ONLY because no detection is ever ignored (the exporter writes one
// difficulty and no don't-care region): with KITTI's neighbouring classes or don't-care areas an unmatched detection may or may
// not count as an FP depending on the threshold, and a per-detection bit cannot say that.
#include "common.h"
#include "ap_kitti.h"
#include "box_iou.h"

#include <limits.h>

namespace dpft {

constexpr int kApMaxN = 1024, kApMaxM = 256, kApMaxC = 16, kApMaxK = 8, kApMaxR = 101;
// counters (int64): [0] record cursor, [1] queries dropped for a NaN score, [2] records refused for lack of capacity,
// [3] true-positive errors that did not fit the fixed point (the *_tp entries only), [16 + c] ground-truth count of class c
constexpr int kApCursor = 0, kApNan = 1, kApOverflow = 2, kApTpSat = 3, kApNpos = 16;

struct ApArgs {
    const float *cls, *center, *size, *angle;      // (B,N,C) (B,N,3) (B,N,3) (B,N,2)
    const float* gt_box;                           // (B,Mmax,8)
    const int32_t* gt_id;                          // (B,Mmax)
    const int32_t* counts;                         // (B)
    double* pair;                                  // (B,N,Mmax,2): bev, 3d
    int4* records;                                 // (capacity): score bits, frame, query | class << 16, TP bits
    unsigned long long* counters;
    double thr[kApMaxK];
    int kind[kApMaxK];                             // 0 bev, 1 3d
    float roi[6];
    int has_roi;
    float min_score;
    long long capacity;
    int first_frame;
    int B, N, Mmax, C, K;
};

constexpr int kApMaxGroupB = 64, kApMaxAxes = 3, kApMaxAxisValues = 16, kApMaxGroups = 32, kApFrameRow = 2 + kApMaxC;
// description storage of a frame: a device pointer to >= 3 elements of one of four types, or three doubles by value
constexpr int kApDescF32 = 0, kApDescF64 = 1, kApDescI32 = 2, kApDescI64 = 3, kApDescHost = 4;

struct ApGroupArgs {
    const void* desc[kApMaxGroupB];                // per sample: the description on the device (types 0..3)
    double host[kApMaxGroupB * 3];                 // per sample: the description by value (type 4)
    unsigned char type[kApMaxGroupB];
    int32_t* frames;                               // (frame capacity, kApFrameRow): frame, group mask, npos[0..15]
    long long frame_base;                          // rows written by earlier updates
    int n_axes;
    int col[kApMaxAxes], count[kApMaxAxes];        // description column and number of values of every selected axis
    int value[kApMaxAxes][kApMaxAxisValues];       // group 1 + (values of earlier axes) + i holds the frames with value[s][i]
};

// bit 0 = "all"; a non-finite value or one outside the axis's values sets no bit of that axis
__device__ __forceinline__ unsigned ap_group_mask(const ApGroupArgs& g, int b) {
    const int t = g.type[b];
    const void* p = g.desc[b];
    unsigned mask = 1u;
    int bit = 1;
    for (int s = 0; s < g.n_axes; ++s) {
        const int col = g.col[s];
        double v;
        if (t == kApDescHost) v = g.host[b * 3 + col];
        else if (t == kApDescF32) v = (double)((const float*)p)[col];
        else if (t == kApDescF64) v = ((const double*)p)[col];
        else if (t == kApDescI32) v = (double)((const int32_t*)p)[col];
        else v = (double)((const long long*)p)[col];
        if (fabs(v) <= 1.7976931348623157e308) {                        // (false for a NaN)
            v = trunc(v);                                               // int(): towards zero, as the exporter reads it
            for (int i = 0; i < g.count[s]; ++i)
                if (v == (double)g.value[s][i]) mask |= 1u << (bit + i);
        }
        bit += g.count[s];
    }
    return mask;
}

struct ApTpArgs {
    long long* err;                                // (capacity, 4): ate, aze, ase, aoe as rint(e * 2^32) at the record's position
    int ref_k;                                     // the reference combination
    int fold_pi;                                   // aoe = min(aoe, pi - aoe)
};

constexpr double kApTpScale = 4294967296.0, kApTpLimit = 1048576.0;      // 2^32 units per metre (or radian); |e| < 2^20
constexpr long long kApTpSaturated = 1ll << 52;

// The four errors of a (detection, target) pair in fp64 straight from the fp32 inputs; the operation order is part of the
// definition (dpft_amd/evaluation/dataset_ap.py; tests/dataset_ap_tp_ref.py restates it).
__device__ inline void ap_tp_errors(const float* ce1, const float* sz1, const float* an1, const float* ce2, const float* sz2,
                                    const float* an2, int fold_pi, double* e) {
    const double dx = (double)ce1[0] - (double)ce2[0], dy = (double)ce1[1] - (double)ce2[1];
    e[0] = sqrt(dx * dx + dy * dy);
    e[1] = fabs((double)ce1[2] - (double)ce2[2]);
    const double l1 = sz1[0], w1 = sz1[1], h1 = sz1[2], l2 = sz2[0], w2 = sz2[1], h2 = sz2[2];
    const double P = fmin(l1, l2) * fmin(w1, w2) * fmin(h1, h2);
    const double v1 = l1 * w1 * h1, v2 = l2 * w2 * h2;
    e[2] = 1.0 - P / (v1 + v2 - P);
    const double r1 = hypot((double)an1[0], (double)an1[1]), r2 = hypot((double)an2[0], (double)an2[1]);
    const double s1 = (double)an1[0] / r1, c1 = (double)an1[1] / r1, s2 = (double)an2[0] / r2, c2 = (double)an2[1] / r2;
    const double t = atan2(fabs(s1 * c2 - c1 * s2), c1 * c2 + s1 * s2);
    e[3] = fold_pi ? fmin(t, 3.141592653589793 - t) : t;
}

// rint(e * 2^32), half to even; a value that is not finite or not below 2^20 in magnitude stores 2^52 and counts in `sat`
__device__ __forceinline__ long long ap_tp_quantise(double e, int& sat) {
    if (!(fabs(e) < kApTpLimit)) { ++sat; return kApTpSaturated; }
    return (long long)rint(e * kApTpScale);
}

__device__ __forceinline__ bool ap_in_roi(const ApArgs& a, const float* c) {
    if (!a.has_roi) return true;
    return (a.roi[0] < c[0]) && (c[0] < a.roi[1]) && (a.roi[2] < c[1]) && (c[1] < a.roi[3]) && (a.roi[4] < c[2]) && (c[2] < a.roi[5]);
}

__global__ __launch_bounds__(128) void ap_pair_kernel(ApArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)a.B * a.N * a.Mmax) return;
    const int j = (int)(idx % a.Mmax);
    const int64_t bn = idx / a.Mmax;
    const int b = (int)(bn / a.N);
    double bev = 0, d3 = 0;
    if (j < a.counts[b]) {
        const int gc = a.gt_id[(int64_t)b * a.Mmax + j];
        const float* g = a.gt_box + ((int64_t)b * a.Mmax + j) * 8;
        float best;
        if (gc != 0 && ap_argmax(a.cls + bn * a.C, a.C, best) == gc && ap_in_roi(a, g) && ap_in_roi(a, a.center + bn * 3))
            ap_iou_pair(a.center + bn * 3, a.size + bn * 3, a.angle + bn * 2, g, g + 3, g + 6, bev, d3);
    }
    a.pair[idx * 2 + 0] = bev;
    a.pair[idx * 2 + 1] = d3;
}

// The two KITTI walks of combination k by one wave (the protocol: dpft_amd/evaluation/dataset_ap.py).  Every loop is bounded by M
// or D and nothing waits on another wave; the bits go into tp[] with LDS atomics like the walk's own.
__device__ __forceinline__ void ap_kitti_walks(const ApArgs& a, const double* pair, const unsigned long long* key,
                                               const float* score, const unsigned char* cand, const unsigned* tcand, unsigned* tp,
                                               int D, int M, int k, int lane) {
    const double thr = a.thr[k];
    const int kd = a.kind[k];
    // ---- pass 1: targets in ascending index; each takes the first unassigned detection in (score desc, query asc) order with
    //      IoU > thr and score >= 0 (the tool's pass-1 score threshold).  Lane holds the assigned bits of the sorted detections
    //      lane, lane + 64, ...: D <= 1024 gives 16 bits ----
    unsigned taken = 0;
    for (int j = 0; j < M; ++j) {
        if (!((tcand[j] >> k) & 1u)) continue;                          // (uniform over the wave)
        for (int ch = 0; ch * 64 < D; ++ch) {
            const int i = ch * 64 + lane;
            bool ok = false;
            if (i < D && ((cand[i] >> k) & 1) && !((taken >> ch) & 1u)) {
                const unsigned q = (unsigned)key[i];
                ok = score[q] >= 0.f && pair[((int64_t)q * a.Mmax + j) * 2 + kd] > thr;
            }
            const unsigned long long bal = __ballot(ok);
            if (bal) {
                if (lane == __ffsll((long long)bal) - 1) {
                    taken |= 1u << ch;
                    atomicOr(&tp[i], 0x100u << k);
                }
                break;
            }
        }
    }
    // ---- pass 2: the detections enter in score order; lane holds targets lane + 64 t with the query and the IoU of the detection
    //      matched to each.  The entering detection goes to the lowest target (from `start`) that is above the threshold and is
    //      free, or holds a smaller IoU, or an equal one from a higher query; a displaced detection is offered on from the next
    //      target.  The chain ends at a free target (the entering detection gets its bit) or when nobody takes (no bit) ----
    int mq[4] = {-1, -1, -1, -1};
    double mv[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < D; ++i) {
        if (!((cand[i] >> k) & 1)) continue;                            // (uniform over the wave)
        int xq = (int)(unsigned)key[i];
        int start = 0;
        for (int step = 0; step < M; ++step) {                          // (every step moves `start` up: at most M)
            const double* row = pair + (int64_t)xq * a.Mmax * 2 + kd;
            int bj = INT_MAX;
            double bv = 0.0;
#pragma unroll
            for (int t = 3; t >= 0; --t) {                              // (descending: the lowest taking target of the lane stays)
                const int j = lane + 64 * t;
                if (j >= start && j < M) {
                    const double v = row[2 * j];
                    if (v > thr && (mq[t] < 0 || v > mv[t] || (v == mv[t] && xq < mq[t]))) { bj = j; bv = v; }
                }
            }
            int lo = bj;
            for (int o = 32; o > 0; o >>= 1) lo = min(lo, __shfl_xor(lo, o));
            if (lo == INT_MAX) break;
            int old = -1;
            if (lane == (lo & 63)) {                                    // (this lane's bj is lo: the lowest of the wave is the lane's lowest)
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (t == (lo >> 6)) { old = mq[t]; mq[t] = xq; mv[t] = bv; }
            }
            old = __shfl(old, lo & 63);
            if (old < 0) {
                if (lane == 0) atomicOr(&tp[i], 0x10000u << k);
                break;
            }
            xq = old;
            start = lo + 1;
        }
    }
}

// `g` is a compile-time null in ap_match_kernel: the frame row below exists in the *_groups kernels only; `t` is one in the kernels
// without true-positive errors: the matched target index and the error rows exist in the *_tp kernels only; `kitti` is a template
// argument, false in the four kernels without the KITTI walks: nothing of the walks is instantiated in them and `tcand`, which only
// the `if constexpr (kitti)` parts touch, takes no LDS there (the kernels' assembly and LDS sizes were compared with the ones from
// before the walks existed when this was written: equal); in the *_kitti kernels `t` is a runtime null
template <bool kitti>
__device__ __forceinline__ void ap_match_body(const ApArgs& a, const ApGroupArgs* g, const ApTpArgs* t) {
    __shared__ unsigned long long key[kApMaxN];      // (score descending, query ascending) as one ascending integer
    __shared__ float score[kApMaxN];
    __shared__ unsigned tp[kApMaxN];                 // per sorted detection: bit k = TP of combination k
    __shared__ unsigned char label[kApMaxN];
    __shared__ unsigned char cand[kApMaxN];          // per sorted detection: bit k = some target lies above threshold k
    __shared__ unsigned char match[kApMaxN];         // per sorted detection: the target the reference combination took (t only)
    __shared__ unsigned tcand[kApMaxM];              // per target: bit k = some detection lies above threshold k (kitti only)
    __shared__ int npos[kApMaxC];
    __shared__ int s_D, s_nan;
    __shared__ long long s_base;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.N, C = a.C, M = min(a.counts[b], a.Mmax);
    if (tid < kApMaxC) npos[tid] = 0;
    if (tid == 0) { s_D = 0; s_nan = 0; }
    __syncthreads();
    // ---- detections of the frame (compacted in arrival order: the sort below fixes the order) and ground-truth counts ----
    for (int n = tid; n < N; n += 256) {
        float s;
        const int l = ap_argmax(a.cls + ((int64_t)b * N + n) * C, C, s);
        label[n] = (unsigned char)l;
        score[n] = s;
        if (l == 0) continue;
        if (s != s) { atomicAdd(&s_nan, 1); continue; }
        if (!(s >= a.min_score) || !ap_in_roi(a, a.center + ((int64_t)b * N + n) * 3)) continue;
        unsigned u = __float_as_uint(s);
        if (u == 0x80000000u) u = 0u;                                   // -0 orders as +0
        const unsigned ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
        key[atomicAdd(&s_D, 1)] = ((unsigned long long)(~ord) << 32) | (unsigned)n;
    }
    for (int j = tid; j < M; j += 256) {
        const int c = a.gt_id[(int64_t)b * a.Mmax + j];
        if (c > 0 && c < C && ap_in_roi(a, a.gt_box + ((int64_t)b * a.Mmax + j) * 8)) atomicAdd(&npos[c], 1);
    }
    __syncthreads();
    const int D = s_D;
    int P = 1;
    while (P < D) P <<= 1;
    for (int i = D + tid; i < P; i += 256) key[i] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {                                  // bitonic sort, ascending
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
    // ---- which detections have a candidate at all (the walk below only stops at those) ----
    const double* pair = a.pair + (int64_t)b * N * a.Mmax * 2;
    if constexpr (kitti) {
        for (int j = tid; j < M; j += 256) tcand[j] = 0u;
        __syncthreads();
    }
    for (int i = tid; i < D; i += 256) {
        const double* row = pair + (int64_t)(unsigned)key[i] * a.Mmax * 2;
        unsigned bits = 0;
        for (int j = 0; j < M; ++j) {
            const double v0 = row[2 * j], v1 = row[2 * j + 1];
            unsigned seen = 0;
            if constexpr (kitti) { seen = bits; bits = 0; }            // (this target's bits alone, for its side of the table)
            for (int k = 0; k < a.K; ++k)
                if ((a.kind[k] ? v1 : v0) > a.thr[k]) bits |= 1u << k;
            if constexpr (kitti) {
                if (bits) atomicOr(&tcand[j], bits);
                bits |= seen;
            }
        }
        cand[i] = (unsigned char)bits;
        tp[i] = 0u;
    }
    __syncthreads();
    // ---- greedy assignment in score order: one wave per combination, lane holds targets lane, lane + 64, ... ----
    for (int k = wave; k < a.K; k += 4) {
        const double thr = a.thr[k];
        const int kd = a.kind[k];
        unsigned assigned = 0;
        for (int i = 0; i < D; ++i) {
            if (!((cand[i] >> k) & 1)) continue;                        // (uniform over the wave)
            const double* row = pair + (int64_t)(unsigned)key[i] * a.Mmax * 2 + kd;
            double bv = -1.0;
            int bj = INT_MAX;
            for (int t = 0; t < 4; ++t) {
                const int j = lane + 64 * t;
                if (j < M && !((assigned >> t) & 1)) {
                    const double v = row[2 * j];
                    if (v > thr && v > bv) { bv = v; bj = j; }
                }
            }
            for (int o = 32; o > 0; o >>= 1) {                          // largest IoU, ties to the lower target index
                const double ov = __shfl_xor(bv, o);
                const int oj = __shfl_xor(bj, o);
                if (ov > bv || (ov == bv && oj < bj)) { bv = ov; bj = oj; }
            }
            if (bj != INT_MAX) {
                if (lane == (bj & 63)) assigned |= 1u << (bj >> 6);
                if (lane == 0) atomicOr(&tp[i], 1u << k);
                if (t && k == t->ref_k && lane == 0) match[i] = (unsigned char)bj;
            }
        }
        if constexpr (kitti) ap_kitti_walks(a, pair, key, score, cand, tcand, tp, D, M, k, lane);
    }
    __syncthreads();
    // ---- append: one cursor atomic per workgroup ----
    if (tid == 0) {
        s_base = D > 0 ? (long long)atomicAdd(a.counters + kApCursor, (unsigned long long)D) : 0;
        if (s_nan) atomicAdd(a.counters + kApNan, (unsigned long long)s_nan);
    }
    if (tid < C && npos[tid]) atomicAdd(a.counters + kApNpos + tid, (unsigned long long)npos[tid]);
    __syncthreads();
    const long long base = s_base;
    for (int i = tid; i < D; i += 256) {
        const long long pos = base + i;
        if (pos >= a.capacity) { atomicAdd(a.counters + kApOverflow, 1ull); continue; }      // (the host sizes the store: never)
        const int q = (int)(unsigned)key[i];
        a.records[pos] = make_int4((int)__float_as_uint(score[q]), a.first_frame + b, q | ((int)label[q] << 16), (int)tp[i]);
        if (t) {                                                        // (non-TP rows are zeros: no stale bytes travel)
            long long v[4] = {0, 0, 0, 0};
            if ((tp[i] >> t->ref_k) & 1u) {
                const float* gb = a.gt_box + ((int64_t)b * a.Mmax + match[i]) * 8;
                const int64_t bn = (int64_t)b * N + q;
                double e[4];
                int sat = 0;
                ap_tp_errors(a.center + bn * 3, a.size + bn * 3, a.angle + bn * 2, gb, gb + 3, gb + 6, t->fold_pi, e);
                for (int x = 0; x < 4; ++x) v[x] = ap_tp_quantise(e[x], sat);
                if (sat) atomicAdd(a.counters + kApTpSat, (unsigned long long)sat);
            }
            longlong2* row = reinterpret_cast<longlong2*>(t->err + pos * 4);
            row[0] = make_longlong2(v[0], v[1]);
            row[1] = make_longlong2(v[2], v[3]);
        }
    }
    if (g && tid < kApFrameRow) {                                       // (the host sized the frame store: frame_base + B rows fit)
        int32_t* row = g->frames + (g->frame_base + b) * kApFrameRow;
        row[tid] = tid == 0 ? a.first_frame + b : tid == 1 ? (int32_t)ap_group_mask(*g, b) : npos[tid - 2];
    }
}

__global__ __launch_bounds__(256) void ap_match_kernel(ApArgs a) { ap_match_body<false>(a, nullptr, nullptr); }

__global__ __launch_bounds__(256) void ap_match_groups_kernel(ApArgs a, ApGroupArgs g) { ap_match_body<false>(a, &g, nullptr); }

__global__ __launch_bounds__(256) void ap_match_tp_kernel(ApArgs a, ApTpArgs t) { ap_match_body<false>(a, nullptr, &t); }

__global__ __launch_bounds__(256) void ap_match_groups_tp_kernel(ApArgs a, ApGroupArgs g, ApTpArgs t) { ap_match_body<false>(a, &g, &t); }

// the match pass with the two KITTI walks; has_t = 0: no true-positive errors (a runtime null)
__global__ __launch_bounds__(256) void ap_match_kitti_kernel(ApArgs a, ApTpArgs t, int has_t) {
    ap_match_body<true>(a, nullptr, has_t ? &t : nullptr);
}

__global__ __launch_bounds__(256) void ap_match_kitti_groups_kernel(ApArgs a, ApGroupArgs g, ApTpArgs t, int has_t) {
    ap_match_body<true>(a, &g, has_t ? &t : nullptr);
}

struct ApFinalArgs {
    const int4* rec;                       // ordered by (class, score desc, frame, query)
    const long long* class_start;          // (C + 1): records of class c are [class_start[c], class_start[c + 1])
    const unsigned long long* counters;
    double *ap, *npos, *tp_total;          // (C-1,K) (C-1) (C-1,K)
    long long n;
    int C, K, R;
};

__global__ __launch_bounds__(256) void ap_finalize_kernel(ApFinalArgs a) {
    __shared__ unsigned long long bins[kApMaxR + 1];
    __shared__ int wsum[4];
    const int c = 1 + blockIdx.x / a.K, k = blockIdx.x % a.K, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long s = min(max(a.class_start[c], 0ll), a.n), e = min(max(a.class_start[c + 1], s), a.n);
    const long long np = (long long)a.counters[kApNpos + c];
    for (int i = tid; i <= a.R; i += 256) bins[i] = 0ull;
    __syncthreads();
    long long carry = 0;
    for (long long base = s; base < e; base += 256) {
        const long long p = base + tid;
        const bool bit = p < e && ((a.rec[p].w >> k) & 1);
        const unsigned long long bal = __ballot(bit);
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int off = 0, tot = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) off += wsum[w];
            tot += wsum[w];
        }
        // only TP positions can raise a bin: an FP position has the TP count of the last TP before it and a lower precision
        if (bit && np > 0) {
            const long long TP = carry + off + __popcll(bal & ((2ull << lane) - 1ull));
            long long idx = TP * a.R / np;                              // largest i with i / R <= TP / npos
            if (idx > a.R) idx = a.R;
            const double prec = (double)TP / (double)(p - s + 1);
            // precisions are non-negative: their bit patterns order as integers
            if (idx >= 1) atomicMax(&bins[idx], (unsigned long long)__double_as_longlong(prec));
        }
        carry += tot;
        __syncthreads();
    }
    if (tid == 0) {
        double env = 0, sum = 0;
        for (int i = a.R; i >= 1; --i) {                                // suffix maximum
            env = fmax(env, __longlong_as_double((long long)bins[i]));
            bins[i] = (unsigned long long)__double_as_longlong(env);
        }
        for (int i = 1; i <= a.R; ++i) sum += __longlong_as_double((long long)bins[i]);
        const int o = (c - 1) * a.K + k;
        a.ap[o] = np > 0 ? sum / (double)a.R : __longlong_as_double(0x7ff8000000000000ll);
        a.tp_total[o] = (double)carry;
        if (k == 0) a.npos[c - 1] = (double)np;
    }
}

struct ApGroupFinalArgs {
    const int4* rec;                       // ordered by (class, score desc, frame, query)
    const unsigned* rec_groups;            // (n): group mask of every record's frame, in the same order
    const long long* class_start;          // (C + 1)
    const int32_t* frames;                 // (F, kApFrameRow)
    double *ap, *npos, *tp_total, *nframes, *bad;      // (G,C-1,K) (G,C-1) (G,C-1,K) (G) (1)
    long long n, F;
    unsigned axis_mask[kApMaxAxes];        // the bits of every selected axis
    int n_axes, G, C, K, R;
};

// blocks 0..G-1: frames and ground truth of group g (integer sums: exact in fp64); block G: frames without a group on some axis
__global__ __launch_bounds__(256) void ap_group_frames_kernel(ApGroupFinalArgs a) {
    __shared__ unsigned long long acc[kApMaxC + 1];
    const int g = blockIdx.x, tid = threadIdx.x;
    if (tid <= kApMaxC) acc[tid] = 0ull;
    __syncthreads();
    if (g == a.G) {
        unsigned long long bad = 0;
        for (long long f = tid; f < a.F; f += 256) {
            const unsigned m = (unsigned)a.frames[f * kApFrameRow + 1];
            bool miss = false;
            for (int s = 0; s < a.n_axes; ++s) miss |= (m & a.axis_mask[s]) == 0u;
            bad += miss;
        }
        if (bad) atomicAdd(&acc[0], bad);
        __syncthreads();
        if (tid == 0) a.bad[0] = (double)acc[0];
        return;
    }
    unsigned long long cnt = 0, np[kApMaxC];
#pragma unroll
    for (int c = 0; c < kApMaxC; ++c) np[c] = 0;
    for (long long f = tid; f < a.F; f += 256) {
        const int32_t* row = a.frames + f * kApFrameRow;
        if (!(((unsigned)row[1] >> g) & 1u)) continue;
        ++cnt;
#pragma unroll
        for (int c = 1; c < kApMaxC; ++c) np[c] += (unsigned long long)(unsigned)row[2 + c];
    }
    if (cnt) atomicAdd(&acc[0], cnt);
#pragma unroll
    for (int c = 1; c < kApMaxC; ++c)
        if (np[c]) atomicAdd(&acc[1 + c], np[c]);
    __syncthreads();
    if (tid == 0) a.nframes[g] = (double)acc[0];
    if (tid >= 1 && tid < a.C) a.npos[g * (a.C - 1) + tid - 1] = (double)acc[1 + tid];
}

// ap_finalize_kernel restricted to the records of group g: rank and TP count are prefix sums over the members
__global__ __launch_bounds__(256) void ap_finalize_groups_kernel(ApGroupFinalArgs a) {
    __shared__ unsigned long long bins[kApMaxR + 1];
    __shared__ int wmem[4], wtp[4];
    const int k = blockIdx.x % a.K, gc = blockIdx.x / a.K, c = 1 + gc % (a.C - 1), g = gc / (a.C - 1);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long s = min(max(a.class_start[c], 0ll), a.n), e = min(max(a.class_start[c + 1], s), a.n);
    const long long np = (long long)a.npos[g * (a.C - 1) + c - 1];
    for (int i = tid; i <= a.R; i += 256) bins[i] = 0ull;
    __syncthreads();
    long long carry = 0, rank0 = 0;
    for (long long base = s; base < e; base += 256) {
        const long long p = base + tid;
        const bool mem = p < e && ((a.rec_groups[p] >> g) & 1u);
        const bool bit = mem && ((a.rec[p].w >> k) & 1);
        const unsigned long long balm = __ballot(mem), bal = __ballot(bit);
        if (lane == 0) { wmem[wave] = __popcll(balm); wtp[wave] = __popcll(bal); }
        __syncthreads();
        int off = 0, tot = 0, offm = 0, totm = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) { off += wtp[w]; offm += wmem[w]; }
            tot += wtp[w];
            totm += wmem[w];
        }
        if (bit && np > 0) {
            const unsigned long long upto = (2ull << lane) - 1ull;
            const long long TP = carry + off + __popcll(bal & upto);
            const long long rank = rank0 + offm + __popcll(balm & upto);        // members up to and including p
            long long idx = TP * a.R / np;
            if (idx > a.R) idx = a.R;
            const double prec = (double)TP / (double)rank;
            if (idx >= 1) atomicMax(&bins[idx], (unsigned long long)__double_as_longlong(prec));
        }
        carry += tot;
        rank0 += totm;
        __syncthreads();
    }
    if (tid == 0) {
        double env = 0, sum = 0;
        for (int i = a.R; i >= 1; --i) {
            env = fmax(env, __longlong_as_double((long long)bins[i]));
            bins[i] = (unsigned long long)__double_as_longlong(env);
        }
        for (int i = 1; i <= a.R; ++i) sum += __longlong_as_double((long long)bins[i]);
        const int o = (g * (a.C - 1) + c - 1) * a.K + k;
        a.ap[o] = np > 0 ? sum / (double)a.R : __longlong_as_double(0x7ff8000000000000ll);
        a.tp_total[o] = (double)carry;
    }
}

struct ApTpFinalArgs {
    const int4* rec;                       // ordered by (class, score desc, frame, query)
    const long long* err;                  // (n, 4): the error rows in the same order
    const unsigned* rec_groups;            // (n) group mask of every record's frame, or null: every record is a member
    const long long* class_start;          // (C + 1)
    const unsigned long long* counters;    // ground truth per class (without groups)
    const double* group_npos;              // (G, C-1) ground truth per group and class (with groups)
    double *tp_err, *tp_points;            // (G, C-1, 4) (G, C-1)
    long long n;
    int G, C, k, R, i_min;
};

// One workgroup per (group, class).  T = TPs of the reference combination so far, S = their integer error sums so far (inclusive
// block scans, carried across trips of 256 records); the TP with count T serves the recall points floor((T-1) R / npos) < i <=
// floor(T R / npos) with the cumulative means S / 2^32 / T: every point has one writer.  The class's error is the mean of the
// served points i >= i_min, summed in ascending i.
__global__ __launch_bounds__(256) void ap_finalize_tp_kernel(ApTpFinalArgs a) {
    __shared__ double table[(kApMaxR + 1) * 4];
    __shared__ unsigned char served[kApMaxR + 1];
    __shared__ int wmem[4], wtp[4];
    __shared__ unsigned long long wsum[4][4];
    const int c = 1 + blockIdx.x % (a.C - 1), g = blockIdx.x / (a.C - 1), k = a.k;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long s = min(max(a.class_start[c], 0ll), a.n), e = min(max(a.class_start[c + 1], s), a.n);
    const long long np = a.rec_groups ? (long long)a.group_npos[g * (a.C - 1) + c - 1] : (long long)a.counters[kApNpos + c];
    for (int i = tid; i <= a.R; i += 256) served[i] = 0;
    __syncthreads();
    long long carry = 0;
    unsigned long long csum[4] = {0ull, 0ull, 0ull, 0ull};              // (unsigned: a sum of saturated rows may wrap, the host
    for (long long base = s; base < e; base += 256) {                  //  reports those as NaN)
        const long long p = base + tid;
        const bool mem = p < e && (!a.rec_groups || ((a.rec_groups[p] >> g) & 1u));
        const bool bit = mem && ((a.rec[p].w >> k) & 1);
        unsigned long long v[4] = {0ull, 0ull, 0ull, 0ull};
        if (bit) {
            const longlong2* row = reinterpret_cast<const longlong2*>(a.err + p * 4);
            const longlong2 r0 = row[0], r1 = row[1];
            v[0] = (unsigned long long)r0.x; v[1] = (unsigned long long)r0.y;
            v[2] = (unsigned long long)r1.x; v[3] = (unsigned long long)r1.y;
        }
        for (int o = 1; o < 64; o <<= 1) {                              // inclusive scan over the wave
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const unsigned long long u = __shfl_up(v[x], o);
                if (lane >= o) v[x] += u;
            }
        }
        const unsigned long long bal = __ballot(bit);
        if (lane == 63) {
#pragma unroll
            for (int x = 0; x < 4; ++x) wsum[wave][x] = v[x];
        }
        if (lane == 0) wtp[wave] = __popcll(bal);
        __syncthreads();
        int off = 0, tot = 0;
        unsigned long long osum[4] = {0ull, 0ull, 0ull, 0ull}, tsum[4] = {0ull, 0ull, 0ull, 0ull};
        for (int w = 0; w < 4; ++w) {
            if (w < wave) off += wtp[w];
            tot += wtp[w];
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                if (w < wave) osum[x] += wsum[w][x];
                tsum[x] += wsum[w][x];
            }
        }
        if (bit && np > 0) {
            const long long T = carry + off + __popcll(bal & ((2ull << lane) - 1ull));
            const long long lo = (T - 1) * a.R / np;
            long long hi = T * a.R / np;
            if (hi > a.R) hi = a.R;
            for (long long i = lo + 1; i <= hi; ++i) {
#pragma unroll
                for (int x = 0; x < 4; ++x)
                    table[i * 4 + x] = (double)(long long)(csum[x] + osum[x] + v[x]) / kApTpScale / (double)T;
                served[i] = 1;
            }
        }
        carry += tot;
#pragma unroll
        for (int x = 0; x < 4; ++x) csum[x] += tsum[x];
        __syncthreads();
    }
    if (tid < 4) {
        double sum = 0;
        int count = 0;
        for (int i = a.i_min; i <= a.R; ++i)
            if (served[i]) { sum += table[i * 4 + tid]; ++count; }
        const int o = g * (a.C - 1) + c - 1;
        a.tp_err[o * 4 + tid] = count > 0 ? sum / (double)count : __longlong_as_double(0x7ff8000000000000ll);
        if (tid == 0) a.tp_points[o] = (double)count;
    }
}

struct ApKittiFinalArgs {
    const int4* rec;                       // ordered by (class, score desc, frame, query)
    const unsigned* rec_groups;            // (n) group mask of every record's frame, or null: every record is a member
    const long long* class_start;          // (C + 1)
    const unsigned long long* counters;    // ground truth per class (without groups)
    const double* group_npos;              // (G, C-1) ground truth per group and class (with groups)
    double *ap40, *ap11;                   // (G, C-1, K)
    double *prec, *recall, *thresholds, *tp, *fp;      // (G, C-1, K, 41)
    int32_t* nthr;                         // (G, C-1, K)
    long long n;
    int G, C, K;
};

// One workgroup per (group, class, combination) over the member records, three trips over them:
//  A  n1 = number of pass-1 bits; thread 0 then picks the ranks of the <= 41 thresholds (ap_kitti_ranks: a function of n1 and npos);
//  B  block prefix sum of the pass-1 bit: the record whose rank was picked gives the threshold its score;
//  C  every member goes into the bin of the first threshold its score reaches (thresholds descend, equal ones leave the later bin
//     empty), with its pass-2 bit beside it: integer counts.  Their running sums over the bins are A = the detections with
//     score >= s up to the END of the threshold's tie group and TP = the pass-2 bits among them; FP = A - TP.
// Then prec = TP / A, rec = TP / G, suffix maximum, AP (R40) and AP11, summed in ascending i by one thread.
__global__ __launch_bounds__(256) void ap_finalize_kitti_kernel(ApKittiFinalArgs a) {
    __shared__ int wsum[4];
    __shared__ long long ranks[kApKittiPoints];
    __shared__ float thr[kApKittiPoints];
    __shared__ unsigned long long cnt_a[kApKittiPoints], cnt_tp[kApKittiPoints];
    __shared__ int s_nt;
    const int k = blockIdx.x % a.K, gc = blockIdx.x / a.K, c = 1 + gc % (a.C - 1), g = gc / (a.C - 1);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long s = min(max(a.class_start[c], 0ll), a.n), e = min(max(a.class_start[c + 1], s), a.n);
    const long long np = a.rec_groups ? (long long)a.group_npos[g * (a.C - 1) + c - 1] : (long long)a.counters[kApNpos + c];
    if (tid < kApKittiPoints) { cnt_a[tid] = 0ull; cnt_tp[tid] = 0ull; thr[tid] = 0.f; }
    // ---- A ----
    long long n1 = 0;
    for (long long base = s; base < e; base += 256) {
        const long long p = base + tid;
        const bool mem = p < e && (!a.rec_groups || ((a.rec_groups[p] >> g) & 1u));
        const bool bit = mem && ((a.rec[p].w >> (8 + k)) & 1);
        const unsigned long long bal = __ballot(bit);
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        for (int w = 0; w < 4; ++w) n1 += wsum[w];
        __syncthreads();
    }
    if (tid == 0) s_nt = np > 0 ? ap_kitti_ranks(n1, np, ranks) : 0;
    __syncthreads();
    const int nt = s_nt;
    // ---- B ----
    long long carry = 0;
    for (long long base = s; base < e && nt > 0; base += 256) {
        const long long p = base + tid;
        const bool mem = p < e && (!a.rec_groups || ((a.rec_groups[p] >> g) & 1u));
        const bool bit = mem && ((a.rec[p].w >> (8 + k)) & 1);
        const unsigned long long bal = __ballot(bit);
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int off = 0, tot = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) off += wsum[w];
            tot += wsum[w];
        }
        if (bit) {
            const long long rank = carry + off + __popcll(bal & ((2ull << lane) - 1ull)) - 1;      // 0-based
            for (int t = 0; t < nt; ++t)
                if (ranks[t] == rank) thr[t] = __int_as_float(a.rec[p].x);
        }
        carry += tot;
        __syncthreads();
    }
    __syncthreads();
    // ---- C ----
    for (long long base = s; base < e && nt > 0; base += 256) {
        const long long p = base + tid;
        const bool mem = p < e && (!a.rec_groups || ((a.rec_groups[p] >> g) & 1u));
        int bin = nt;
        bool hit = false;
        if (mem) {
            const int4 r = a.rec[p];
            const float sc = __int_as_float(r.x);
            hit = (r.w >> (16 + k)) & 1;
            for (int t = nt - 1; t >= 0; --t)
                if (sc >= thr[t]) bin = t;                              // the first threshold the score reaches
        }
        const unsigned long long hits = __ballot(hit);
        unsigned long long todo = __ballot(bin < nt);
        while (todo) {                                                  // one LDS atomic pair per distinct bin of the wave
            const int leader = __ffsll((long long)todo) - 1;
            const int lb = __shfl(bin, leader);
            const unsigned long long same = __ballot(bin == lb) & todo;
            if (lane == leader) {
                atomicAdd(&cnt_a[lb], (unsigned long long)__popcll(same));
                atomicAdd(&cnt_tp[lb], (unsigned long long)__popcll(same & hits));
            }
            todo &= ~same;
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int o = (g * (a.C - 1) + c - 1) * a.K + k;
        double* prec = a.prec + (long long)o * kApKittiPoints;
        double* recall = a.recall + (long long)o * kApKittiPoints;
        double* thrs = a.thresholds + (long long)o * kApKittiPoints;
        double* tp = a.tp + (long long)o * kApKittiPoints;
        double* fp = a.fp + (long long)o * kApKittiPoints;
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        double env[kApKittiPoints];
        unsigned long long A = 0, T = 0;
        for (int t = 0; t < kApKittiPoints; ++t) {
            if (t < nt) {
                A += cnt_a[t];
                T += cnt_tp[t];
                prec[t] = (double)T / (double)A;
                recall[t] = (double)T / (double)np;
                thrs[t] = (double)thr[t];
                tp[t] = (double)T;
                fp[t] = (double)(A - T);
            } else {
                prec[t] = 0.0; recall[t] = 0.0; thrs[t] = nan; tp[t] = 0.0; fp[t] = 0.0;
            }
        }
        double m = 0.0;
        for (int t = kApKittiPoints - 1; t >= 0; --t) {                 // suffix maximum
            m = fmax(m, prec[t]);
            env[t] = m;
        }
        double s40 = 0.0, s11 = 0.0;
        for (int t = 1; t <= 40; ++t) s40 += env[t];
        for (int t = 0; t <= 40; t += 4) s11 += env[t];
        a.ap40[o] = np > 0 ? s40 / 40.0 : nan;
        a.ap11[o] = np > 0 ? s11 / 11.0 : nan;
        a.nthr[o] = nt;
    }
}

static bool ap_sizes_ok(int B, int N, int Mmax, int C) {
    return B > 0 && N > 0 && N <= kApMaxN && Mmax > 0 && Mmax <= kApMaxM && C >= 2 && C <= kApMaxC;
}

}  // namespace dpft

using namespace dpft;

extern "C" int64_t dpft_dataset_ap_scratch_bytes(int32_t B, int32_t N, int32_t Mmax) {
    if (!(B > 0 && N > 0 && N <= kApMaxN && Mmax > 0 && Mmax <= kApMaxM)) {
        set_error("dataset_ap_scratch_bytes: sizes out of range (N <= %d, Mmax <= %d)", kApMaxN, kApMaxM);
        return -1;
    }
    return (int64_t)B * N * Mmax * 2 * (int64_t)sizeof(double);
}

// argument checks and ApArgs shared by the two update entries
static int ap_fill_update(ApArgs& a, const float* cls, const float* center, const float* size, const float* angle,
                          const float* gt_box, const int32_t* gt_id, const int32_t* counts, const double* iou_thrs,
                          const int32_t* kinds, int32_t K, const float* roi6, float min_score, void* scratch, void* records,
                          int64_t capacity, int64_t reserved, int64_t* counters, int32_t first_frame, int32_t B, int32_t N,
                          int32_t Mmax, int32_t C) {
    DPFT_REQUIRE(cls && center && size && angle && gt_box && gt_id && counts && iou_thrs && kinds && scratch && records && counters,
                 "dataset_ap_update: null argument");
    DPFT_REQUIRE(ap_sizes_ok(B, N, Mmax, C), "dataset_ap_update: sizes out of range (N <= %d, Mmax <= %d, 2 <= C <= %d)", kApMaxN,
                 kApMaxM, kApMaxC);
    DPFT_REQUIRE(K >= 1 && K <= kApMaxK, "dataset_ap_update: 1..%d combinations, got %d", kApMaxK, K);
    DPFT_REQUIRE(reserved >= 0 && capacity - reserved >= (int64_t)B * N,
                 "dataset_ap_update: record store too small (capacity %lld, reserved %lld, this batch up to %lld)",
                 (long long)capacity, (long long)reserved, (long long)B * N);
    DPFT_REQUIRE(((uintptr_t)records & 15) == 0 && ((uintptr_t)scratch & 7) == 0 && ((uintptr_t)counters & 7) == 0,
                 "dataset_ap_update: records need 16-byte, scratch and counters 8-byte alignment");
    memset(&a, 0, sizeof(a));
    for (int k = 0; k < K; ++k) {
        DPFT_REQUIRE(iou_thrs[k] > 0.0 && iou_thrs[k] < 1.0 && (kinds[k] == 0 || kinds[k] == 1),
                     "dataset_ap_update: combination %d needs a threshold inside (0, 1) and kind 0 (bev) or 1 (3d)", k);
        a.thr[k] = iou_thrs[k];
        a.kind[k] = kinds[k];
    }
    if (roi6) {
        for (int i = 0; i < 6; ++i) {
            DPFT_REQUIRE(roi6[i] == roi6[i] && fabsf(roi6[i]) != INFINITY, "dataset_ap_update: roi[%d] is not finite", i);
            a.roi[i] = roi6[i];
        }
        a.has_roi = 1;
    }
    a.cls = cls; a.center = center; a.size = size; a.angle = angle; a.gt_box = gt_box; a.gt_id = gt_id; a.counts = counts;
    a.pair = (double*)scratch; a.records = (int4*)records; a.counters = (unsigned long long*)counters;
    a.min_score = min_score; a.capacity = capacity; a.first_frame = first_frame;
    a.B = B; a.N = N; a.Mmax = Mmax; a.C = C; a.K = K;
    return DPFT_OK;
}

// the true-positive arguments of the *_tp entries (checked before anything is launched)
static int ap_fill_tp(ApTpArgs& t, void* tp_errors, int32_t ref_k, int32_t fold_pi, int32_t K) {
    DPFT_REQUIRE(tp_errors, "dataset_ap_update_tp: null argument");
    DPFT_REQUIRE(((uintptr_t)tp_errors & 15) == 0, "dataset_ap_update_tp: the error rows need 16-byte alignment");
    DPFT_REQUIRE(ref_k >= 0 && ref_k < K, "dataset_ap_update_tp: the reference combination must be one of the %d, got %d", K, ref_k);
    DPFT_REQUIRE(fold_pi == 0 || fold_pi == 1, "dataset_ap_update_tp: fold_pi must be 0 or 1, got %d", fold_pi);
    t.err = (long long*)tp_errors; t.ref_k = ref_k; t.fold_pi = fold_pi;
    return DPFT_OK;
}

// the two launches of an update without groups; `t` = null: no true-positive errors
static int ap_update(const float* cls, const float* center, const float* size, const float* angle, const float* gt_box,
                     const int32_t* gt_id, const int32_t* counts, const double* iou_thrs, const int32_t* kinds, int32_t K,
                     const float* roi6, float min_score, void* scratch, void* records, int64_t capacity, int64_t reserved,
                     int64_t* counters, int32_t first_frame, int32_t B, int32_t N, int32_t Mmax, int32_t C, const ApTpArgs* t,
                     bool kitti, dpft_stream_t stream) {
    ApArgs a;
    int rc = ap_fill_update(a, cls, center, size, angle, gt_box, gt_id, counts, iou_thrs, kinds, K, roi6, min_score, scratch, records,
                            capacity, reserved, counters, first_frame, B, N, Mmax, C);
    if (rc) return rc;
    const int64_t total = (int64_t)B * N * Mmax;
    hipLaunchKernelGGL(ap_pair_kernel, dim3(cdiv(total, 128)), dim3(128), 0, (hipStream_t)stream, a);
    rc = check_launch("dataset_ap_update pairs");
    if (rc) return rc;
    if (kitti) {
        ApTpArgs none;
        memset(&none, 0, sizeof(none));
        hipLaunchKernelGGL(ap_match_kitti_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a, t ? *t : none, t ? 1 : 0);
    } else if (t) hipLaunchKernelGGL(ap_match_tp_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a, *t);
    else hipLaunchKernelGGL(ap_match_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("dataset_ap_update");
}

extern "C" int dpft_dataset_ap_update_f32(const float* cls, const float* center, const float* size, const float* angle,
                                          const float* gt_box, const int32_t* gt_id, const int32_t* counts,
                                          const double* iou_thrs, const int32_t* kinds, int32_t K, const float* roi6,
                                          float min_score, void* scratch, void* records, int64_t capacity, int64_t reserved,
                                          int64_t* counters, int32_t first_frame, int32_t B, int32_t N, int32_t Mmax,
                                          int32_t C, dpft_stream_t stream) {
    return ap_update(cls, center, size, angle, gt_box, gt_id, counts, iou_thrs, kinds, K, roi6, min_score, scratch, records, capacity,
                     reserved, counters, first_frame, B, N, Mmax, C, nullptr, false, stream);
}

extern "C" int dpft_dataset_ap_update_tp_f32(const float* cls, const float* center, const float* size, const float* angle,
                                             const float* gt_box, const int32_t* gt_id, const int32_t* counts,
                                             const double* iou_thrs, const int32_t* kinds, int32_t K, const float* roi6,
                                             float min_score, void* scratch, void* records, int64_t capacity, int64_t reserved,
                                             int64_t* counters, int32_t first_frame, int32_t B, int32_t N, int32_t Mmax,
                                             int32_t C, void* tp_errors, int32_t ref_k, int32_t fold_pi, dpft_stream_t stream) {
    ApTpArgs t;
    int rc = ap_fill_tp(t, tp_errors, ref_k, fold_pi, K);
    if (rc) return rc;
    return ap_update(cls, center, size, angle, gt_box, gt_id, counts, iou_thrs, kinds, K, roi6, min_score, scratch, records, capacity,
                     reserved, counters, first_frame, B, N, Mmax, C, &t, false, stream);
}

// the two launches of an update with groups; `t` = null: no true-positive errors
static int ap_update_groups(const float* cls, const float* center, const float* size, const float* angle, const float* gt_box,
                            const int32_t* gt_id, const int32_t* counts, const double* iou_thrs, const int32_t* kinds, int32_t K,
                            const float* roi6, float min_score, void* scratch, void* records, int64_t capacity, int64_t reserved,
                            int64_t* counters, int32_t first_frame, int32_t B, int32_t N, int32_t Mmax, int32_t C,
                            const void* const* desc_ptrs, const int32_t* desc_types, const double* desc_host,
                            const int32_t* axis_cols, const int32_t* axis_counts, const int32_t* axis_values, int32_t n_axes,
                            void* frames, int64_t frame_capacity, int64_t frames_before, const ApTpArgs* t, bool kitti,
                            dpft_stream_t stream) {
    DPFT_REQUIRE(desc_ptrs && desc_types && frames, "dataset_ap_update_groups: null argument");
    DPFT_REQUIRE(n_axes == 0 || (axis_cols && axis_counts && axis_values), "dataset_ap_update_groups: null axis tables");
    ApArgs a;
    int rc = ap_fill_update(a, cls, center, size, angle, gt_box, gt_id, counts, iou_thrs, kinds, K, roi6, min_score, scratch, records,
                            capacity, reserved, counters, first_frame, B, N, Mmax, C);
    if (rc) return rc;
    DPFT_REQUIRE(B <= kApMaxGroupB, "dataset_ap_update_groups: at most %d frames per update, got %d", kApMaxGroupB, B);
    DPFT_REQUIRE(n_axes >= 0 && n_axes <= kApMaxAxes, "dataset_ap_update_groups: 0..%d axes, got %d", kApMaxAxes, n_axes);
    DPFT_REQUIRE(frames_before >= 0 && frame_capacity - frames_before >= (int64_t)B && ((uintptr_t)frames & 3) == 0,
                 "dataset_ap_update_groups: frame store too small or unaligned (capacity %lld, %lld rows before, this batch %d)",
                 (long long)frame_capacity, (long long)frames_before, B);
    ApGroupArgs g;
    memset(&g, 0, sizeof(g));
    int groups = 1;
    for (int s = 0; s < n_axes; ++s) {
        DPFT_REQUIRE(axis_cols[s] >= 0 && axis_cols[s] < 3 && axis_counts[s] >= 1 && axis_counts[s] <= kApMaxAxisValues,
                     "dataset_ap_update_groups: axis %d needs a description column 0..2 and 1..%d values", s, kApMaxAxisValues);
        g.col[s] = axis_cols[s];
        g.count[s] = axis_counts[s];
        for (int i = 0; i < axis_counts[s]; ++i) g.value[s][i] = axis_values[s * kApMaxAxisValues + i];
        groups += axis_counts[s];
    }
    DPFT_REQUIRE(groups <= kApMaxGroups, "dataset_ap_update_groups: %d groups, at most %d", groups, kApMaxGroups);
    static const int desc_bytes[4] = {4, 8, 4, 8};
    for (int b = 0; b < B; ++b) {
        const int t = desc_types[b];
        DPFT_REQUIRE(t >= kApDescF32 && t <= kApDescHost, "dataset_ap_update_groups: description type %d of sample %d (0..4)", t, b);
        if (t == kApDescHost) {
            DPFT_REQUIRE(desc_host, "dataset_ap_update_groups: sample %d has its description by value but desc_host is null", b);
            for (int i = 0; i < 3; ++i) g.host[b * 3 + i] = desc_host[b * 3 + i];
        } else {
            DPFT_REQUIRE(desc_ptrs[b] && ((uintptr_t)desc_ptrs[b] & (uintptr_t)(desc_bytes[t] - 1)) == 0,
                         "dataset_ap_update_groups: description pointer of sample %d is null or unaligned", b);
            g.desc[b] = desc_ptrs[b];
        }
        g.type[b] = (unsigned char)t;
    }
    g.frames = (int32_t*)frames;
    g.frame_base = frames_before;
    g.n_axes = n_axes;
    const int64_t total = (int64_t)B * N * Mmax;
    hipLaunchKernelGGL(ap_pair_kernel, dim3(cdiv(total, 128)), dim3(128), 0, (hipStream_t)stream, a);
    rc = check_launch("dataset_ap_update_groups pairs");
    if (rc) return rc;
    if (kitti) {
        ApTpArgs none;
        memset(&none, 0, sizeof(none));
        hipLaunchKernelGGL(ap_match_kitti_groups_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a, g, t ? *t : none, t ? 1 : 0);
    } else if (t) hipLaunchKernelGGL(ap_match_groups_tp_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a, g, *t);
    else hipLaunchKernelGGL(ap_match_groups_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a, g);
    return check_launch("dataset_ap_update_groups");
}

extern "C" int dpft_dataset_ap_update_groups_f32(const float* cls, const float* center, const float* size, const float* angle,
        const float* gt_box, const int32_t* gt_id, const int32_t* counts, const double* iou_thrs, const int32_t* kinds, int32_t K,
        const float* roi6, float min_score, void* scratch, void* records, int64_t capacity, int64_t reserved, int64_t* counters,
        int32_t first_frame, int32_t B, int32_t N, int32_t Mmax, int32_t C, const void* const* desc_ptrs, const int32_t* desc_types,
        const double* desc_host, const int32_t* axis_cols, const int32_t* axis_counts, const int32_t* axis_values, int32_t n_axes,
        void* frames, int64_t frame_capacity, int64_t frames_before, dpft_stream_t stream) {
    return ap_update_groups(cls, center, size, angle, gt_box, gt_id, counts, iou_thrs, kinds, K, roi6, min_score, scratch, records,
                            capacity, reserved, counters, first_frame, B, N, Mmax, C, desc_ptrs, desc_types, desc_host, axis_cols,
                            axis_counts, axis_values, n_axes, frames, frame_capacity, frames_before, nullptr, false, stream);
}

extern "C" int dpft_dataset_ap_update_groups_tp_f32(const float* cls, const float* center, const float* size, const float* angle,
        const float* gt_box, const int32_t* gt_id, const int32_t* counts, const double* iou_thrs, const int32_t* kinds, int32_t K,
        const float* roi6, float min_score, void* scratch, void* records, int64_t capacity, int64_t reserved, int64_t* counters,
        int32_t first_frame, int32_t B, int32_t N, int32_t Mmax, int32_t C, const void* const* desc_ptrs, const int32_t* desc_types,
        const double* desc_host, const int32_t* axis_cols, const int32_t* axis_counts, const int32_t* axis_values, int32_t n_axes,
        void* frames, int64_t frame_capacity, int64_t frames_before, void* tp_errors, int32_t ref_k, int32_t fold_pi,
        dpft_stream_t stream) {
    ApTpArgs t;
    int rc = ap_fill_tp(t, tp_errors, ref_k, fold_pi, K);
    if (rc) return rc;
    return ap_update_groups(cls, center, size, angle, gt_box, gt_id, counts, iou_thrs, kinds, K, roi6, min_score, scratch, records,
                            capacity, reserved, counters, first_frame, B, N, Mmax, C, desc_ptrs, desc_types, desc_host, axis_cols,
                            axis_counts, axis_values, n_axes, frames, frame_capacity, frames_before, &t, false, stream);
}

// The update with the KITTI walks: frames = null -> without groups (the description and axis arguments are not read), tp_errors =
// null -> without true-positive errors (ref_k and fold_pi are not read).  The same two launches either way.
extern "C" int dpft_dataset_ap_update_kitti_f32(const float* cls, const float* center, const float* size, const float* angle,
        const float* gt_box, const int32_t* gt_id, const int32_t* counts, const double* iou_thrs, const int32_t* kinds, int32_t K,
        const float* roi6, float min_score, void* scratch, void* records, int64_t capacity, int64_t reserved, int64_t* counters,
        int32_t first_frame, int32_t B, int32_t N, int32_t Mmax, int32_t C, const void* const* desc_ptrs, const int32_t* desc_types,
        const double* desc_host, const int32_t* axis_cols, const int32_t* axis_counts, const int32_t* axis_values, int32_t n_axes,
        void* frames, int64_t frame_capacity, int64_t frames_before, void* tp_errors, int32_t ref_k, int32_t fold_pi,
        dpft_stream_t stream) {
    ApTpArgs t;
    if (tp_errors) {
        int rc = ap_fill_tp(t, tp_errors, ref_k, fold_pi, K);
        if (rc) return rc;
    }
    if (!frames)
        return ap_update(cls, center, size, angle, gt_box, gt_id, counts, iou_thrs, kinds, K, roi6, min_score, scratch, records,
                         capacity, reserved, counters, first_frame, B, N, Mmax, C, tp_errors ? &t : nullptr, true, stream);
    return ap_update_groups(cls, center, size, angle, gt_box, gt_id, counts, iou_thrs, kinds, K, roi6, min_score, scratch, records,
                            capacity, reserved, counters, first_frame, B, N, Mmax, C, desc_ptrs, desc_types, desc_host, axis_cols,
                            axis_counts, axis_values, n_axes, frames, frame_capacity, frames_before, tp_errors ? &t : nullptr, true,
                            stream);
}

extern "C" int dpft_dataset_ap_finalize_f64(const void* records_sorted, int64_t n_records, const int64_t* class_start,
                                            const int64_t* counters, int32_t C, int32_t K, int32_t R, double* ap,
                                            double* npos, double* tp_total, dpft_stream_t stream) {
    DPFT_REQUIRE(records_sorted && class_start && counters && ap && npos && tp_total, "dataset_ap_finalize: null argument");
    DPFT_REQUIRE(n_records >= 0 && C >= 2 && C <= kApMaxC && K >= 1 && K <= kApMaxK && R >= 2 && R <= kApMaxR,
                 "dataset_ap_finalize: sizes out of range (2 <= C <= %d, 1 <= K <= %d, 2 <= R <= %d)", kApMaxC, kApMaxK, kApMaxR);
    ApFinalArgs a;
    a.rec = (const int4*)records_sorted; a.class_start = (const long long*)class_start;
    a.counters = (const unsigned long long*)counters; a.ap = ap; a.npos = npos; a.tp_total = tp_total;
    a.n = n_records; a.C = C; a.K = K; a.R = R;
    hipLaunchKernelGGL(ap_finalize_kernel, dim3((C - 1) * K), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("dataset_ap_finalize");
}

extern "C" int dpft_dataset_ap_finalize_groups_f64(const void* records_sorted, const uint32_t* record_groups, int64_t n_records,
                                                   const int64_t* class_start, const void* frames, int64_t n_frames,
                                                   const uint32_t* axis_masks, int32_t n_axes, int32_t G, int32_t C, int32_t K,
                                                   int32_t R, double* ap, double* npos, double* tp_total, double* nframes,
                                                   double* bad, dpft_stream_t stream) {
    DPFT_REQUIRE(records_sorted && record_groups && class_start && frames && ap && npos && tp_total && nframes && bad,
                 "dataset_ap_finalize_groups: null argument");
    DPFT_REQUIRE(n_records >= 0 && n_frames >= 0 && C >= 2 && C <= kApMaxC && K >= 1 && K <= kApMaxK && R >= 2 && R <= kApMaxR,
                 "dataset_ap_finalize_groups: sizes out of range (2 <= C <= %d, 1 <= K <= %d, 2 <= R <= %d)", kApMaxC, kApMaxK,
                 kApMaxR);
    DPFT_REQUIRE(G >= 1 && G <= kApMaxGroups && n_axes >= 0 && n_axes <= kApMaxAxes && (n_axes == 0 || axis_masks),
                 "dataset_ap_finalize_groups: 1..%d groups and 0..%d axes (with their masks), got %d and %d", kApMaxGroups,
                 kApMaxAxes, G, n_axes);
    ApGroupFinalArgs a;
    memset(&a, 0, sizeof(a));
    for (int s = 0; s < n_axes; ++s) a.axis_mask[s] = axis_masks[s];
    a.rec = (const int4*)records_sorted; a.rec_groups = record_groups; a.class_start = (const long long*)class_start;
    a.frames = (const int32_t*)frames; a.ap = ap; a.npos = npos; a.tp_total = tp_total; a.nframes = nframes; a.bad = bad;
    a.n = n_records; a.F = n_frames; a.n_axes = n_axes; a.G = G; a.C = C; a.K = K; a.R = R;
    hipLaunchKernelGGL(ap_group_frames_kernel, dim3(G + 1), dim3(256), 0, (hipStream_t)stream, a);
    int rc = check_launch("dataset_ap_finalize_groups frames");
    if (rc) return rc;
    hipLaunchKernelGGL(ap_finalize_groups_kernel, dim3(G * (C - 1) * K), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("dataset_ap_finalize_groups");
}

// argument checks and launch shared by the two true-positive finalize entries (record_groups = null: without groups)
static int ap_finalize_tp(const char* who, const void* records_sorted, const int64_t* tp_errors_sorted, const uint32_t* record_groups,
                          int64_t n_records, const int64_t* class_start, const int64_t* counters, const double* group_npos, int32_t G,
                          int32_t C, int32_t ref_k, int32_t R, int32_t i_min, double* tp_err, double* tp_points,
                          dpft_stream_t stream) {
    DPFT_REQUIRE(records_sorted && tp_errors_sorted && class_start && tp_err && tp_points, "%s: null argument", who);
    DPFT_REQUIRE(n_records >= 0 && C >= 2 && C <= kApMaxC && ref_k >= 0 && ref_k < kApMaxK && R >= 2 && R <= kApMaxR,
                 "%s: sizes out of range (2 <= C <= %d, 0 <= ref_k < %d, 2 <= R <= %d)", who, kApMaxC, kApMaxK, kApMaxR);
    DPFT_REQUIRE(i_min >= 1 && i_min <= R, "%s: the first recall point must lie in 1..R, got %d", who, i_min);
    DPFT_REQUIRE(G >= 1 && G <= kApMaxGroups, "%s: 1..%d groups, got %d", who, kApMaxGroups, G);
    DPFT_REQUIRE(((uintptr_t)records_sorted & 15) == 0 && ((uintptr_t)tp_errors_sorted & 15) == 0,
                 "%s: records and error rows need 16-byte alignment", who);
    ApTpFinalArgs a;
    memset(&a, 0, sizeof(a));
    a.rec = (const int4*)records_sorted; a.err = (const long long*)tp_errors_sorted; a.rec_groups = record_groups;
    a.class_start = (const long long*)class_start; a.counters = (const unsigned long long*)counters; a.group_npos = group_npos;
    a.tp_err = tp_err; a.tp_points = tp_points; a.n = n_records; a.G = G; a.C = C; a.k = ref_k; a.R = R; a.i_min = i_min;
    hipLaunchKernelGGL(ap_finalize_tp_kernel, dim3(G * (C - 1)), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch(who);
}

extern "C" int dpft_dataset_ap_finalize_tp_f64(const void* records_sorted, const int64_t* tp_errors_sorted, int64_t n_records,
                                               const int64_t* class_start, const int64_t* counters, int32_t C, int32_t ref_k,
                                               int32_t R, int32_t i_min, double* tp_err, double* tp_points, dpft_stream_t stream) {
    DPFT_REQUIRE(counters, "dataset_ap_finalize_tp: null argument");
    return ap_finalize_tp("dataset_ap_finalize_tp", records_sorted, tp_errors_sorted, nullptr, n_records, class_start, counters,
                          nullptr, 1, C, ref_k, R, i_min, tp_err, tp_points, stream);
}

extern "C" int dpft_dataset_ap_finalize_tp_groups_f64(const void* records_sorted, const int64_t* tp_errors_sorted,
                                                      const uint32_t* record_groups, int64_t n_records, const int64_t* class_start,
                                                      const double* group_npos, int32_t G, int32_t C, int32_t ref_k, int32_t R,
                                                      int32_t i_min, double* tp_err, double* tp_points, dpft_stream_t stream) {
    DPFT_REQUIRE(record_groups && group_npos, "dataset_ap_finalize_tp_groups: null argument");
    return ap_finalize_tp("dataset_ap_finalize_tp_groups", records_sorted, tp_errors_sorted, record_groups, n_records, class_start,
                          nullptr, group_npos, G, C, ref_k, R, i_min, tp_err, tp_points, stream);
}

// argument checks and launch shared by the two KITTI finalize entries (record_groups = null: without groups)
static int ap_finalize_kitti(const char* who, const void* records_sorted, const uint32_t* record_groups, int64_t n_records,
                             const int64_t* class_start, const int64_t* counters, const double* group_npos, int32_t G, int32_t C,
                             int32_t K, double* ap40, double* ap11, double* prec, double* rec, double* thresholds, double* tp,
                             double* fp, int32_t* nthr, dpft_stream_t stream) {
    DPFT_REQUIRE(records_sorted && class_start && ap40 && ap11 && prec && rec && thresholds && tp && fp && nthr, "%s: null argument",
                 who);
    DPFT_REQUIRE(n_records >= 0 && C >= 2 && C <= kApMaxC && K >= 1 && K <= kApMaxK,
                 "%s: sizes out of range (2 <= C <= %d, 1 <= K <= %d)", who, kApMaxC, kApMaxK);
    DPFT_REQUIRE(G >= 1 && G <= kApMaxGroups, "%s: 1..%d groups, got %d", who, kApMaxGroups, G);
    DPFT_REQUIRE(((uintptr_t)records_sorted & 15) == 0, "%s: records need 16-byte alignment", who);
    ApKittiFinalArgs a;
    memset(&a, 0, sizeof(a));
    a.rec = (const int4*)records_sorted; a.rec_groups = record_groups; a.class_start = (const long long*)class_start;
    a.counters = (const unsigned long long*)counters; a.group_npos = group_npos; a.ap40 = ap40; a.ap11 = ap11; a.prec = prec;
    a.recall = rec; a.thresholds = thresholds; a.tp = tp; a.fp = fp; a.nthr = nthr; a.n = n_records; a.G = G; a.C = C; a.K = K;
    hipLaunchKernelGGL(ap_finalize_kitti_kernel, dim3(G * (C - 1) * K), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch(who);
}

extern "C" int dpft_dataset_ap_finalize_kitti_f64(const void* records_sorted, int64_t n_records, const int64_t* class_start,
                                                  const int64_t* counters, int32_t C, int32_t K, double* ap40, double* ap11,
                                                  double* prec, double* rec, double* thresholds, double* tp, double* fp,
                                                  int32_t* nthr, dpft_stream_t stream) {
    DPFT_REQUIRE(counters, "dataset_ap_finalize_kitti: null argument");
    return ap_finalize_kitti("dataset_ap_finalize_kitti", records_sorted, nullptr, n_records, class_start, counters, nullptr, 1, C, K,
                             ap40, ap11, prec, rec, thresholds, tp, fp, nthr, stream);
}

extern "C" int dpft_dataset_ap_finalize_kitti_groups_f64(const void* records_sorted, const uint32_t* record_groups,
                                                         int64_t n_records, const int64_t* class_start, const double* group_npos,
                                                         int32_t G, int32_t C, int32_t K, double* ap40, double* ap11, double* prec,
                                                         double* rec, double* thresholds, double* tp, double* fp, int32_t* nthr,
                                                         dpft_stream_t stream) {
    DPFT_REQUIRE(record_groups && group_npos, "dataset_ap_finalize_kitti_groups: null argument");
    return ap_finalize_kitti("dataset_ap_finalize_kitti_groups", records_sorted, record_groups, n_records, class_start, nullptr,
                             group_npos, G, C, K, ap40, ap11, prec, rec, thresholds, tp, fp, nthr, stream);
}

// The host side of ap_kitti_ranks, for the tests: the same function the finalize kernel runs, no GPU involved.
extern "C" int dpft_dataset_ap_kitti_ranks(int64_t n1, int64_t npos, int64_t* ranks) {
    DPFT_REQUIRE(ranks, "dataset_ap_kitti_ranks: null argument");
    DPFT_REQUIRE(n1 >= 0 && npos >= 1 && n1 <= npos, "dataset_ap_kitti_ranks: 0 <= n1 <= npos and npos >= 1, got %lld and %lld",
                 (long long)n1, (long long)npos);
    long long picked[kApKittiPoints];
    const int nt = ap_kitti_ranks(n1, npos, picked);
    for (int t = 0; t < nt; ++t) ranks[t] = picked[t];
    return nt;
}
