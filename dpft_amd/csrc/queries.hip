// Learned query points (src/dprt/models/queries/learnable.py:103-128): the (Q,3) parameter, repeated over the batch and passed
// through the querent's coordinate transformation (src/dprt/models/utils/transformations.py:212-281), and the way back:
//   center[b][q] = f(queries[q])                          f = identity | spher2cart (radians | degrees)
//   dqueries[q]  = J_f(queries[q])^T  sum_b dcenter[b][q]
// The batch sum runs in ONE thread per query, b ascending: no atomics, the same bits every call.
#include "common.h"

namespace dpft {

constexpr float kDeg2Rad = 0.017453292519943295f;

struct SpherAngles {
    float cp, sp, cr, sr;      // cos / sin of azimuth (phi) and elevation (roh)
};
__device__ __forceinline__ SpherAngles spher_angles(float phi, float roh, int mode) {
    if (mode == DPFT_QUERY_SPHER2CART_DEG) {
        phi *= kDeg2Rad;
        roh *= kDeg2Rad;
    }
    return {cosf(phi), sinf(phi), cosf(roh), sinf(roh)};
}

__global__ __launch_bounds__(256) void query_center_fwd_kernel(const float* __restrict__ queries, int mode,
                                                               float* __restrict__ center, int B, int Q) {
    const int i = blockIdx.x * 256 + threadIdx.x;      // (b, q) row
    if (i >= B * Q) return;
    const float* qp = queries + (size_t)(i % Q) * 3;
    float x = qp[0], y = qp[1], z = qp[2];
    if (mode != DPFT_QUERY_IDENTITY) {
        const float r = x;
        const SpherAngles t = spher_angles(y, z, mode);
        x = r * t.cp * t.cr;
        y = r * t.sp * t.cr;
        z = r * t.sr;
    }
    float* c = center + (size_t)i * 3;
    c[0] = x; c[1] = y; c[2] = z;
}

__global__ __launch_bounds__(256) void query_center_bwd_kernel(const float* __restrict__ dcenter,
                                                               const float* __restrict__ queries, int mode,
                                                               float* __restrict__ dqueries, int B, int Q) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    float dx = 0.f, dy = 0.f, dz = 0.f;
    for (int b = 0; b < B; ++b) {
        const float* d = dcenter + ((size_t)b * Q + q) * 3;
        dx += d[0]; dy += d[1]; dz += d[2];
    }
    if (mode != DPFT_QUERY_IDENTITY) {
        const float* qp = queries + (size_t)q * 3;
        const float r = qp[0], k = mode == DPFT_QUERY_SPHER2CART_DEG ? kDeg2Rad : 1.f;
        const SpherAngles t = spher_angles(qp[1], qp[2], mode);
        const float dr = (dx * t.cp + dy * t.sp) * t.cr + dz * t.sr;
        const float dphi = k * r * t.cr * (dy * t.cp - dx * t.sp);
        const float droh = k * r * (dz * t.cr - (dx * t.cp + dy * t.sp) * t.sr);
        dx = dr; dy = dphi; dz = droh;
    }
    float* g = dqueries + (size_t)q * 3;
    g[0] = dx; g[1] = dy; g[2] = dz;
}

static int query_check(const char* what, int32_t mode, int32_t B, int32_t Q) {
    DPFT_REQUIRE(mode == DPFT_QUERY_IDENTITY || mode == DPFT_QUERY_SPHER2CART_RAD || mode == DPFT_QUERY_SPHER2CART_DEG,
                 "%s: unknown transformation mode %d", what, mode);
    DPFT_REQUIRE(B > 0 && Q > 0 && (int64_t)B * Q * 3 < ((int64_t)1 << 31), "%s: bad shape (B=%d, Q=%d)", what, B, Q);
    return DPFT_OK;
}

}  // namespace dpft

using namespace dpft;

extern "C" int dpft_query_center_fwd_f32(const float* queries, int32_t mode, float* center, int32_t B, int32_t Q,
                                         dpft_stream_t stream) {
    DPFT_REQUIRE(queries && center, "query_center_fwd: null pointer");
    const int rc = query_check("query_center_fwd", mode, B, Q);
    if (rc) return rc;
    hipLaunchKernelGGL(query_center_fwd_kernel, dim3(cdiv((int64_t)B * Q, 256)), dim3(256), 0, (hipStream_t)stream, queries,
                       mode, center, B, Q);
    return check_launch("query_center_fwd");
}

extern "C" int dpft_query_center_bwd_f32(const float* dcenter, const float* queries, int32_t mode, float* dqueries,
                                         int32_t B, int32_t Q, dpft_stream_t stream) {
    DPFT_REQUIRE(dcenter && queries && dqueries, "query_center_bwd: null pointer");
    const int rc = query_check("query_center_bwd", mode, B, Q);
    if (rc) return rc;
    hipLaunchKernelGGL(query_center_bwd_kernel, dim3(cdiv(Q, 256)), dim3(256), 0, (hipStream_t)stream, dcenter, queries, mode,
                       dqueries, B, Q);
    return check_launch("query_center_bwd");
}
