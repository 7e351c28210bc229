// Test-time augmentation: the fusion of T views' outputs (dpft_amd/evaluation/tta.py holds the definition; tests/tta_ref.py restates
// it in numpy fp64).  Per batch, on the caller's stream, no host read-back:
//   gather      one launch copies the T views' class / center / size / angle tensors into the union tensors (B, T N, .), candidate
//               m = t N + n, and un-mirrors the flipped views: the sign BIT of center[1] and angle[0] is flipped (-0 <-> +0, NaNs
//               keep their payload).  float4 where the rows of a view (N w floats) and the pointers allow it.
//   clustering  dpft_nms_f32 on the union (three launches, nms.hip), class-aware, no max_det.  Its scratch keeps the candidates in
//               sorted order (nms_layout.h): query, class, score and the 8 box floats; status names each suppressed candidate's head.
//   vote        one workgroup per frame.  The sorted scores, boxes and each position's head position are staged in LDS (56 KB);
//               one lane per head walks the sorted positions from its own onwards and accumulates its members in fp64 in that order:
//               plain sequential adds, no atomics, nothing depends on which workgroup or lane runs first.  This file is built with
//               -ffp-contract=off: every product and sum rounds as the restatement's does; / and sqrt are IEEE.
// The same input gives the same bits.
#include "common.h"
#include "nms_layout.h"

#include <limits.h>
#include <math.h>

namespace dpft {

constexpr int kTtaMaxM = 1024, kTtaMaxC = 16, kTtaMaxT = DPFT_TTA_MAX_VIEWS;

struct TtaGatherArgs {
    dpft_tta_views v;
    float* dst[4];                 // union class (B,M,C), center (B,M,3), size (B,M,3), angle (B,M,2)
    int width[4], vec[4];          // floats per row; float4 path allowed
    int N, T;
};

// blockIdx.z = tensor, blockIdx.y = (frame, view): a contiguous run of N w floats moves to offset (b T + t) N w of the union
__global__ __launch_bounds__(256) void tta_gather_kernel(const TtaGatherArgs a) {
    const int k = blockIdx.z, w = a.width[k];
    const int b = blockIdx.y / a.T, t = blockIdx.y - b * a.T;
    const float* src = (k == 0 ? a.v.cls[t] : k == 1 ? a.v.center[t] : k == 2 ? a.v.size[t] : a.v.angle[t]);
    const int64_t len = (int64_t)a.N * w;
    src += (int64_t)b * len;
    float* dst = a.dst[k] + ((int64_t)b * a.T + t) * len;
    const int col = (a.v.flip[t] && k != 0 && k != 2) ? (k == 1 ? 1 : 0) : -1;      // the mirrored column of a row, or none
    const int stride = gridDim.x * blockDim.x, i0 = blockIdx.x * blockDim.x + threadIdx.x;
    if (a.vec[k]) {
        const uint4* s4 = (const uint4*)src;
        uint4* d4 = (uint4*)dst;
        for (int64_t i = i0; i < len / 4; i += stride) {
            uint4 x = s4[i];
            if (col >= 0) {
                const int r = (int)((i * 4) % w);                                   // column of x.x
                if (r == col) x.x ^= 0x80000000u;
                if ((r + 1) % w == col) x.y ^= 0x80000000u;
                if ((r + 2) % w == col) x.z ^= 0x80000000u;
                if ((r + 3) % w == col) x.w ^= 0x80000000u;
            }
            d4[i] = x;
        }
    } else {
        const unsigned* s1 = (const unsigned*)src;
        unsigned* d1 = (unsigned*)dst;
        for (int64_t i = i0; i < len; i += stride) {
            unsigned x = s1[i];
            if (col >= 0 && (int)(i % w) == col) x ^= 0x80000000u;
            d1[i] = x;
        }
    }
}

struct TtaVoteArgs {
    const float *center, *size, *angle;      // the union (B,M,3) (B,M,3) (B,M,2)
    const int32_t* status;                   // (B,M) of dpft_nms_f32 on the union
    NmsScratch nms;                          // its scratch: the candidates in sorted order
    float *cls_out, *center_out, *size_out, *angle_out;      // cls_out: dpft_nms_f32's, the head rows are rewritten here
    int32_t* members;                        // (B,M)
    int M, C, T, score_max;
};

__global__ __launch_bounds__(256) void tta_vote_kernel(const TtaVoteArgs a) {
    __shared__ float box[kTtaMaxM * 8];      // sorted order
    __shared__ float score[kTtaMaxM];
    __shared__ short pos_of[kTtaMaxM];       // query -> sorted position
    __shared__ short head[kTtaMaxM];         // sorted position -> sorted position of its cluster's head (itself for a head)
    __shared__ double unit[kTtaMaxM * 2];    // (sin, cos) / sqrt(sin^2 + cos^2): once per candidate, by all lanes, not per walk
    const int b = blockIdx.x, tid = threadIdx.x, M = a.M, C = a.C;
    const int64_t base = (int64_t)b * M;
    const int D = min(a.nms.ndet[b], M);
    for (int i = tid; i < D; i += 256) {
        const float4* bx = (const float4*)(a.nms.box + (base + i) * 8);
        const float4 p0 = bx[0], p1 = bx[1];
        float* o = box + i * 8;
        o[0] = p0.x; o[1] = p0.y; o[2] = p0.z; o[3] = p0.w; o[4] = p1.x; o[5] = p1.y; o[6] = p1.z; o[7] = p1.w;
        score[i] = a.nms.score[base + i];
        const double ms = (double)p1.z, mc = (double)p1.w;
        const double r = sqrt(ms * ms + mc * mc);
        unit[2 * i] = ms / r;
        unit[2 * i + 1] = mc / r;
        const int q = a.nms.sorted[base + i];
        if (q >= 0 && q < M) pos_of[q] = (short)i;
    }
    __syncthreads();
    for (int i = tid; i < D; i += 256) {
        const int q = a.nms.sorted[base + i];
        const int st = (q >= 0 && q < M) ? a.status[base + q] : -2;
        head[i] = (short)((st >= 0 && st < M) ? pos_of[st] : (st == -1 ? i : -1));
    }
    // ---- every row that heads no cluster: the un-mirrored geometry bits; its class row is dpft_nms_f32's already ----
    for (int m = tid; m < M; m += 256) {
        if (a.status[base + m] == -1) continue;
        const unsigned *ce = (const unsigned*)(a.center + (base + m) * 3), *sz = (const unsigned*)(a.size + (base + m) * 3);
        const unsigned* an = (const unsigned*)(a.angle + (base + m) * 2);
        unsigned *ceo = (unsigned*)(a.center_out + (base + m) * 3), *szo = (unsigned*)(a.size_out + (base + m) * 3);
        unsigned* ano = (unsigned*)(a.angle_out + (base + m) * 2);
        for (int k = 0; k < 3; ++k) { ceo[k] = ce[k]; szo[k] = sz[k]; }
        ano[0] = an[0]; ano[1] = an[1];
        a.members[base + m] = 0;
    }
    __syncthreads();
    // ---- one lane per head ----
    for (int i = tid; i < D; i += 256) {
        if (head[i] != i) continue;
        const float* hb = box + i * 8;
        const double hus = unit[2 * i], huc = unit[2 * i + 1];
        double sw = 0.0, ss = 0.0, aw = 0.0, as = 0.0, ac = 0.0, acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        int n = 0;
        for (int j = i; j < D; ++j) {
            if (head[j] != i) continue;
            const float s = score[j];
            const float* mb = box + j * 8;
            const double w = (s > 0.f && s < INFINITY) ? (double)s : 0.0;
            ++n;
            ss = ss + (double)s;
            sw = sw + w;
            for (int k = 0; k < 6; ++k) acc[k] = acc[k] + w * (double)mb[k];
            const double us = unit[2 * j], uc = unit[2 * j + 1];
            if (us * hus + uc * huc < 0.0) continue;      // an opposed heading: no vote on the angle (a NaN compares false)
            aw = aw + w;
            as = as + w * us;
            ac = ac + w * uc;
        }
        const int q = a.nms.sorted[base + i];
        if (q < 0 || q >= M) continue;
        const int64_t row = base + q;
        float o[8];
        for (int k = 0; k < 8; ++k) o[k] = hb[k];
        if (n >= 2 && sw > 0.0) {
            for (int k = 0; k < 6; ++k) o[k] = (float)(acc[k] / sw);
            if (aw > 0.0) { o[6] = (float)(as / aw); o[7] = (float)(ac / aw); }
        }
        for (int k = 0; k < 3; ++k) { a.center_out[row * 3 + k] = o[k]; a.size_out[row * 3 + k] = o[3 + k]; }
        a.angle_out[row * 2] = o[6];
        a.angle_out[row * 2 + 1] = o[7];
        const float fused = a.score_max ? score[i] : (float)(ss / (double)max(n, a.T));
        const int c = a.nms.label[base + i];
        float* crow = a.cls_out + row * C;
        for (int k = 0; k < C; ++k) crow[k] = (k == c) ? fused : 0.f;
        a.members[row] = n;
    }
}

static bool tta_sizes_ok(int64_t B, int64_t N, int64_t T, const char* what) {
    if (!(T >= 2 && T <= kTtaMaxT)) {
        set_error("%s: 2 <= T <= %d views (the identity included), got T %lld", what, kTtaMaxT, (long long)T);
        return false;
    }
    if (!(B >= 0 && B <= 65536 && N >= 0)) {
        set_error("%s: sizes out of range (0 <= B <= 65536, N >= 0), got B %lld, N %lld", what, (long long)B, (long long)N);
        return false;
    }
    if (T * N > kTtaMaxM) {
        set_error("%s: T * N must be <= %d, got T %lld, N %lld (%lld candidates)", what, kTtaMaxM, (long long)T, (long long)N,
                  (long long)(T * N));
        return false;
    }
    return true;
}

}  // namespace dpft

using namespace dpft;

extern "C" int64_t dpft_tta_scratch_bytes(int32_t B, int32_t N, int32_t T) {
    if (!tta_sizes_ok(B, N, T, "tta_scratch_bytes")) return -1;
    if (B == 0 || N == 0) return 0;
    return nms_scratch_size(B, (int64_t)T * N);      // dpft_nms_scratch_bytes(B, T N): the union's clustering
}

extern "C" int dpft_tta_gather_f32(const dpft_tta_views* views, int32_t T, float* cls, float* center, float* size, float* angle,
                                   int32_t B, int32_t N, int32_t C, dpft_stream_t stream) {
    if (!tta_sizes_ok(B, N, T, "tta_gather")) return DPFT_ERR_ARG;
    DPFT_REQUIRE(C >= 2 && C <= kTtaMaxC, "tta_gather: 2 <= C <= %d, got C %d", kTtaMaxC, C);
    DPFT_REQUIRE(views, "tta_gather: null argument (views)");
    DPFT_REQUIRE((int64_t)B * T <= 65535, "tta_gather: B * T must be <= 65535, got B %d, T %d", B, T);
    if (B == 0 || N == 0) return DPFT_OK;
    DPFT_REQUIRE(cls && center && size && angle, "tta_gather: null argument (union tensors)");
    TtaGatherArgs a;
    memset(&a, 0, sizeof(a));
    a.v = *views;
    a.dst[0] = cls; a.dst[1] = center; a.dst[2] = size; a.dst[3] = angle;
    a.width[0] = C; a.width[1] = 3; a.width[2] = 3; a.width[3] = 2;
    a.N = N; a.T = T;
    uintptr_t low[4] = {(uintptr_t)cls, (uintptr_t)center, (uintptr_t)size, (uintptr_t)angle};
    for (int t = 0; t < T; ++t) {
        DPFT_REQUIRE(views->cls[t] && views->center[t] && views->size[t] && views->angle[t], "tta_gather: view %d: null tensor", t);
        const float* src[4] = {views->cls[t], views->center[t], views->size[t], views->angle[t]};
        for (int k = 0; k < 4; ++k) {
            DPFT_REQUIRE(src[k] != a.dst[k], "tta_gather: view %d: a union tensor must not alias its source", t);
            low[k] |= (uintptr_t)src[k];
        }
    }
    for (int t = T; t < kTtaMaxT; ++t) {
        a.v.cls[t] = a.v.center[t] = a.v.size[t] = a.v.angle[t] = nullptr;
        a.v.flip[t] = 0;
    }
    int64_t longest = 0;
    for (int k = 0; k < 4; ++k) {
        const int64_t len = (int64_t)N * a.width[k];
        a.vec[k] = (len % 4 == 0) && (low[k] & 15) == 0;
        longest = std::max(longest, a.vec[k] ? len / 4 : len);
    }
    const unsigned gx = (unsigned)std::min<int64_t>(cdiv(longest, 256), 64);
    hipLaunchKernelGGL(tta_gather_kernel, dim3(gx, (unsigned)(B * T), 4), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("tta gather");
}

extern "C" int dpft_tta_vote_f32(const float* center, const float* size, const float* angle, const int32_t* status,
                                 const void* scratch, int32_t score, int32_t T, float* cls_out, float* center_out, float* size_out,
                                 float* angle_out, int32_t* members, int32_t B, int32_t N, int32_t C, dpft_stream_t stream) {
    if (!tta_sizes_ok(B, N, T, "tta_vote")) return DPFT_ERR_ARG;
    DPFT_REQUIRE(C >= 2 && C <= kTtaMaxC, "tta_vote: 2 <= C <= %d, got C %d", kTtaMaxC, C);
    DPFT_REQUIRE(score == 0 || score == 1, "tta_vote: score 0 (mean) or 1 (max), got %d", score);
    if (B == 0 || N == 0) return DPFT_OK;
    DPFT_REQUIRE(center && size && angle && status && scratch && cls_out && center_out && size_out && angle_out && members,
                 "tta_vote: null argument");
    DPFT_REQUIRE(center_out != center && size_out != size && angle_out != angle, "tta_vote: the outputs must not alias the union");
    DPFT_REQUIRE(((uintptr_t)scratch & 15) == 0, "tta_vote: scratch needs 16-byte alignment");
    TtaVoteArgs a;
    memset(&a, 0, sizeof(a));
    const int M = T * N;
    a.center = center; a.size = size; a.angle = angle; a.status = status;
    a.nms = nms_scratch_layout(const_cast<void*>(scratch), B, M);
    a.cls_out = cls_out; a.center_out = center_out; a.size_out = size_out; a.angle_out = angle_out; a.members = members;
    a.M = M; a.C = C; a.T = T; a.score_max = score;
    hipLaunchKernelGGL(tta_vote_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("tta vote");
}
