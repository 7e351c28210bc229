// On-device input preprocessing of the K-Radar training pipeline, done per sample on 16 CPU worker
// processes in the reference:
//   * camera: torchvision.transforms.functional.resize on the float HWC frame, bilinear, no antialias
//     (src/dprt/datasets/kradar/dataset.py:319-341) == F.interpolate(mode="bilinear", align_corners=False);
//     the u8 variant takes the decoded JPEG bytes directly (4x fewer bytes over PCIe) and yields the same floats.
//   * radar: (v - min_power) / (max_power - min_power) * 255 clipped to [0, 255] (dataset.py:295-317).
// Pure streaming kernels: one thread per output element, NHWC in and out (the layout the backbones consume).
#include "common.h"

namespace dpft {

template <typename T>
__global__ __launch_bounds__(256) void resize_bilinear_kernel(const T* __restrict__ src, float* __restrict__ dst, int B,
                                                               int Hs, int Ws, int Hd, int Wd, int C, float sh,
                                                               float sw) {
    const int64_t total = (int64_t)B * Hd * Wd * C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        int64_t t = i / C;
        const int x = (int)(t % Wd); t /= Wd;
        const int y = (int)(t % Hd);
        const int b = (int)(t / Hd);
        // source index of the area-pixel model (align_corners = False), clamped at 0 like ATen's upsample kernels
        float fy = sh * ((float)y + 0.5f) - 0.5f, fx = sw * ((float)x + 0.5f) - 0.5f;
        fy = fy < 0.f ? 0.f : fy;
        fx = fx < 0.f ? 0.f : fx;
        const int y0 = (int)fy, x0 = (int)fx;
        const int y1 = y0 + (y0 < Hs - 1 ? 1 : 0), x1 = x0 + (x0 < Ws - 1 ? 1 : 0);
        const float ly = fy - (float)y0, lx = fx - (float)x0;
        const T* p = src + (int64_t)b * Hs * Ws * C + c;
        const float v00 = (float)p[((int64_t)y0 * Ws + x0) * C], v01 = (float)p[((int64_t)y0 * Ws + x1) * C];
        const float v10 = (float)p[((int64_t)y1 * Ws + x0) * C], v11 = (float)p[((int64_t)y1 * Ws + x1) * C];
        dst[i] = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
    }
}

__global__ __launch_bounds__(256) void scale_clip_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n,
                                                          float in_lo, float in_hi, float out_lo, float out_hi) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float v = (x[i] - in_lo) / (in_hi - in_lo) * (out_hi - out_lo) + out_lo;
        y[i] = fminf(fmaxf(v, out_lo), out_hi);
    }
}

static int resize_check(const void* src, const float* dst, int B, int Hs, int Ws, int Hd, int Wd, int C) {
    DPFT_REQUIRE(src && dst, "resize_bilinear: null tensor");
    DPFT_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0 && C > 0, "resize_bilinear: non-positive sizes");
    return DPFT_OK;
}

}  // namespace dpft

using namespace dpft;

extern "C" int dpft_resize_bilinear_nhwc_f32(const float* src, float* dst, int32_t B, int32_t Hs, int32_t Ws, int32_t Hd,
                                             int32_t Wd, int32_t C, dpft_stream_t stream) {
    int rc = resize_check(src, dst, B, Hs, Ws, Hd, Wd, C);
    if (rc) return rc;
    const int64_t total = (int64_t)B * Hd * Wd * C;
    hipLaunchKernelGGL(resize_bilinear_kernel<float>, dim3((unsigned)std::min<int64_t>(cdiv(total, 256), kNumCU * 16)),
                       dim3(256), 0, (hipStream_t)stream, src, dst, B, Hs, Ws, Hd, Wd, C, (float)Hs / (float)Hd,
                       (float)Ws / (float)Wd);
    return check_launch("resize_bilinear_f32");
}

extern "C" int dpft_resize_bilinear_nhwc_u8(const uint8_t* src, float* dst, int32_t B, int32_t Hs, int32_t Ws, int32_t Hd,
                                            int32_t Wd, int32_t C, dpft_stream_t stream) {
    int rc = resize_check(src, dst, B, Hs, Ws, Hd, Wd, C);
    if (rc) return rc;
    const int64_t total = (int64_t)B * Hd * Wd * C;
    hipLaunchKernelGGL(resize_bilinear_kernel<uint8_t>, dim3((unsigned)std::min<int64_t>(cdiv(total, 256), kNumCU * 16)),
                       dim3(256), 0, (hipStream_t)stream, src, dst, B, Hs, Ws, Hd, Wd, C, (float)Hs / (float)Hd,
                       (float)Ws / (float)Wd);
    return check_launch("resize_bilinear_u8");
}

extern "C" int dpft_scale_clip_f32(const float* x, float* y, int64_t n, float in_lo, float in_hi, float out_lo,
                                   float out_hi, dpft_stream_t stream) {
    DPFT_REQUIRE(x && y && n > 0, "scale_clip: bad arguments");
    DPFT_REQUIRE(in_hi != in_lo, "scale_clip: empty input range");
    hipLaunchKernelGGL(scale_clip_kernel, dim3((unsigned)std::min<int64_t>(cdiv(n, 256), kNumCU * 16)), dim3(256), 0,
                       (hipStream_t)stream, x, y, n, in_lo, in_hi, out_lo, out_hi);
    return check_launch("scale_clip");
}

// ---------------------------------------------------------------------------------------------------------
// Training augmentation (DESIGN.md section 3 "Training augmentation"): one horizontal flip per sample applied to every view
// and to the labels, a camera zoom / shift about the canvas centre, a photometric step on the camera and a gain on the radar
// maps.  The per-sample parameters are drawn on the host and travel BY VALUE in the kernel arguments, DPFT_AUGMENT_CHUNK
// samples per launch (blockIdx.y = the sample of the chunk: its parameters are wave-uniform reads of the argument block).
// ---------------------------------------------------------------------------------------------------------
namespace dpft {

struct CamSample {
    float kx, cx, ky, cy;      // source centre of output pixel (x, y): ((x + 1/2) kx + cx, (y + 1/2) ky + cy)
    float gain[4], offset;
    int flip, exact, photo;
};
struct CamChunk {
    CamSample s[DPFT_AUGMENT_CHUNK];
};

// The interpolation with the roundings resize_bilinear_kernel has AS COMPILED, spelled out (contraction off, explicit fma) so that
// the bits do not hang on what the compiler makes of this kernel's surroundings: each row fma(lx, right, (1 - lx) left), the
// rows joined by fma(1 - ly, top, ly bottom).  That is the u8 kernel everywhere and the f32 kernel in the unrolled body of its
// grid-stride loop; in the loop's tail -- every element of an output the grid covers in one pass, kNumCU * 16 * 256 elements -- the
// f32 kernel has the bottom row as fma(1 - lx, left, lx right) and the join as two rounded products and a sum (kTail).
template <bool kTail>
__device__ __forceinline__ float resize_interp(float ly, float lx, float v00, float v01, float v10, float v11) {
#pragma clang fp contract(off)
    const float top = __builtin_fmaf(lx, v01, (1.f - lx) * v00);
    if (kTail) {
        const float bottom = __builtin_fmaf(1.f - lx, v10, lx * v11);
        return (1.f - ly) * top + ly * bottom;
    }
    const float bottom = __builtin_fmaf(lx, v11, (1.f - lx) * v10);
    return __builtin_fmaf(1.f - ly, top, ly * bottom);
}

// One thread per OUTPUT PIXEL: coordinates, taps and weights once, then the C <= 4 channels.
template <typename T>
__global__ __launch_bounds__(256) void augment_camera_kernel(const T* __restrict__ src, float* __restrict__ dst, int Hs,
                                                              int Ws, int Hd, int Wd, int C, float sh, float sw,
                                                              const CamChunk chunk) {
    const CamSample& p = chunk.s[blockIdx.y];
    const T* frame = src + (int64_t)blockIdx.y * Hs * Ws * C;
    float* out = dst + (int64_t)blockIdx.y * Hd * Wd * C;
    const int total = Hd * Wd;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int y = i / Wd, x = i - y * Wd;
        float fy, fx;
        bool inside = true;
        if (p.exact) {
            // no zoom, no shift: the resize kernel's own formula at x, or at the mirrored column -- its bits
            const int xs = p.flip ? Wd - 1 - x : x;
            fy = __builtin_fmaf(sh, (float)y + 0.5f, -0.5f);
            fx = __builtin_fmaf(sw, (float)xs + 0.5f, -0.5f);
        } else {
            const float uy = ((float)y + 0.5f) * p.ky + p.cy, ux = ((float)x + 0.5f) * p.kx + p.cx;
            inside = uy >= 0.f && uy <= (float)Hs && ux >= 0.f && ux <= (float)Ws;
            fy = uy - 0.5f;
            fx = ux - 0.5f;
        }
        float* o = out + (int64_t)i * C;
        if (!inside) {      // the source centre lies outside the frame: fill, whatever the photometric parameters
            for (int c = 0; c < C; ++c) o[c] = 0.f;
            continue;
        }
        fy = fy < 0.f ? 0.f : fy;
        fx = fx < 0.f ? 0.f : fx;
        int y0 = (int)fy, x0 = (int)fx;
        y0 = y0 < Hs - 1 ? y0 : Hs - 1;
        x0 = x0 < Ws - 1 ? x0 : Ws - 1;
        const int y1 = y0 + (y0 < Hs - 1 ? 1 : 0), x1 = x0 + (x0 < Ws - 1 ? 1 : 0);
        const float ly = fy - (float)y0, lx = fx - (float)x0;
        const T* p00 = frame + ((int64_t)y0 * Ws + x0) * C;
        const T* p01 = frame + ((int64_t)y0 * Ws + x1) * C;
        const T* p10 = frame + ((int64_t)y1 * Ws + x0) * C;
        const T* p11 = frame + ((int64_t)y1 * Ws + x1) * C;
        for (int c = 0; c < C; ++c) {
            const float v00 = (float)p00[c], v01 = (float)p01[c], v10 = (float)p10[c], v11 = (float)p11[c];
            float v = resize_interp<sizeof(T) == 4>(ly, lx, v00, v01, v10, v11);
            if (p.photo) v = fminf(fmaxf(p.gain[c] * v + p.offset, 0.f), 255.f);
            o[c] = v;
        }
    }
}

struct RadarSample {
    float delta;
    int flip;
};
struct RadarChunk {
    RadarSample s[DPFT_AUGMENT_CHUNK];
};

// scale_clip_kernel's arithmetic on x + delta, read from the mirrored azimuth column (axis 2 of (B,H,W,C)) of a flipped sample
__global__ __launch_bounds__(256) void augment_radar_kernel(const float* __restrict__ x, float* __restrict__ y, int rows, int W,
                                                             int C, int scale, float in_lo, float in_hi, float out_lo,
                                                             float out_hi, const RadarChunk chunk) {
    const RadarSample& p = chunk.s[blockIdx.y];
    const int64_t n = (int64_t)rows * W * C;
    const float* xs = x + (int64_t)blockIdx.y * n;
    float* ys = y + (int64_t)blockIdx.y * n;
    const int wc = W * C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t j = i;
        if (p.flip) {
            const int64_t r = i / wc;
            const int rem = (int)(i - r * wc);
            const int w = rem / C, c = rem - w * C;
            j = r * wc + (int64_t)(W - 1 - w) * C + c;
        }
        float v = xs[j];
        if (scale) {
            if (p.delta != 0.f) v = v + p.delta;
            v = (v - in_lo) / (in_hi - in_lo) * (out_hi - out_lo) + out_lo;
            v = fminf(fmaxf(v, out_lo), out_hi);
        }
        ys[i] = v;
    }
}

struct GeoSample {
    float a, bu, s, bv;      // camera map in canvas units of 1: u' / W = a u / W + bu, v' / H = s v / H + bv
    int flip, pad;
};
struct GeoTable {
    dpft_augment_view view[DPFT_AUGMENT_MAX_VIEWS];
    dpft_augment_labels labels[DPFT_AUGMENT_CHUNK];
    GeoSample s[DPFT_AUGMENT_CHUNK];
    int V, b0;
};

__device__ __forceinline__ float flip_sign(float x) { return x != 0.f ? -x : x; }      // zeros keep their sign (T.any() flags)

// One workgroup per sample of the chunk: T' = F T F, P' = M P diag(1,-1,1,1), labels (y, sin) negated; everything out of place.
__global__ __launch_bounds__(128) void augment_geometry_kernel(const GeoTable t) {
    const int j = blockIdx.x;
    const int64_t b = t.b0 + j;
    const GeoSample& sp = t.s[j];
    const bool flip = sp.flip != 0;
    for (int v = 0; v < t.V; ++v) {
        const dpft_augment_view& vw = t.view[v];
        const float* T = vw.T + b * 16;
        for (int i = threadIdx.x; i < 16; i += blockDim.x) {
            const int r = i >> 2, c = i & 3;
            float x = T[i];
            if (flip && ((r == 1) != (c == 1))) x = flip_sign(x);
            vw.T_out[b * 16 + i] = x;
        }
        const int n = vw.p_rows * 4;
        const float* P = vw.P + b * n;
        const float H = (float)vw.shape[b * vw.shape_stride], W = (float)vw.shape[b * vw.shape_stride + 1];
        float a, bu, s, bv;
        if (vw.zoom) {
            a = sp.a; bu = sp.bu * W; s = sp.s; bv = sp.bv * H;
        } else {
            a = flip ? -1.f : 1.f; bu = flip ? W : 0.f; s = 1.f; bv = 0.f;
        }
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int r = i >> 2, c = i & 3;
            float x = P[i];
            if (r == 0 && !(a == 1.f && bu == 0.f)) x = a * x + bu * P[8 + c];
            if (r == 1 && !(s == 1.f && bv == 0.f)) x = s * x + bv * P[8 + c];
            if (flip && c == 1) x = flip_sign(x);
            vw.P_out[b * n + i] = x;
        }
    }
    const dpft_augment_labels& lb = t.labels[j];
    for (int i = threadIdx.x; i < lb.rows * 3; i += blockDim.x) {
        const float x = lb.center[i];
        lb.center_out[i] = (flip && i % 3 == 1) ? -x : x;
    }
    for (int i = threadIdx.x; i < lb.rows * 2; i += blockDim.x) {
        const float x = lb.angle[i];
        lb.angle_out[i] = (flip && i % 2 == 0) ? -x : x;
    }
}

static int augment_samples_check(const dpft_augment_sample* s, int B, const char* what) {
    DPFT_REQUIRE(s, "%s: null sample parameters", what);
    for (int b = 0; b < B; ++b)
        DPFT_REQUIRE(s[b].s > 0.f && s[b].s < INFINITY && (s[b].a == s[b].s || s[b].a == -s[b].s) &&
                         (s[b].flip != 0) == (s[b].a < 0.f),
                     "%s: sample %d: a must be +-s with s > 0, negative exactly when the sample flips", what, b);
    return DPFT_OK;
}

template <typename T>
static int augment_camera(const T* src, float* dst, int B, int Hs, int Ws, int Hd, int Wd, int C,
                          const dpft_augment_sample* samples, dpft_stream_t stream, const char* what) {
    int rc = resize_check(src, dst, B, Hs, Ws, Hd, Wd, C);
    if (rc) return rc;
    DPFT_REQUIRE(C <= 4, "%s: at most 4 channels (got %d)", what, C);
    DPFT_REQUIRE((int64_t)Hd * Wd < (1ll << 30) && (int64_t)Hs * Ws < (1ll << 30), "%s: frame too large", what);
    rc = augment_samples_check(samples, B, what);
    if (rc) return rc;
    const unsigned gx = (unsigned)std::min<int64_t>(cdiv((int64_t)Hd * Wd, 256), kNumCU * 16);
    for (int b0 = 0; b0 < B; b0 += DPFT_AUGMENT_CHUNK) {
        const int nb = std::min(DPFT_AUGMENT_CHUNK, B - b0);
        CamChunk chunk;
        memset(&chunk, 0, sizeof(chunk));
        for (int j = 0; j < nb; ++j) {
            const dpft_augment_sample& a = samples[b0 + j];
            CamSample& c = chunk.s[j];
            // canvas (u, v) in units of (W, H): u' = a u + bu  =>  source centre = ((x + 1/2) / Wd - bu) / a * Ws
            c.kx = (float)((double)Ws / ((double)Wd * (double)a.a));
            c.cx = (float)(-(double)a.bu / (double)a.a * (double)Ws);
            c.ky = (float)((double)Hs / ((double)Hd * (double)a.s));
            c.cy = (float)(-(double)a.bv / (double)a.s * (double)Hs);
            c.offset = a.offset;
            c.photo = a.offset != 0.f;
            for (int k = 0; k < 4; ++k) {
                c.gain[k] = a.gain[k];
                c.photo |= k < C && a.gain[k] != 1.f;
            }
            c.flip = a.flip != 0;
            c.exact = a.s == 1.f && a.bv == 0.f && a.bu == (a.flip ? 1.f : 0.f);
        }
        hipLaunchKernelGGL(augment_camera_kernel<T>, dim3(gx, (unsigned)nb), dim3(256), 0, (hipStream_t)stream,
                           src + (int64_t)b0 * Hs * Ws * C, dst + (int64_t)b0 * Hd * Wd * C, Hs, Ws, Hd, Wd, C,
                           (float)Hs / (float)Hd, (float)Ws / (float)Wd, chunk);
        rc = check_launch(what);
        if (rc) return rc;
    }
    return DPFT_OK;
}

}  // namespace dpft

extern "C" int dpft_augment_camera_nhwc_f32(const float* src, float* dst, int32_t B, int32_t Hs, int32_t Ws, int32_t Hd,
                                            int32_t Wd, int32_t C, const dpft_augment_sample* samples,
                                            dpft_stream_t stream) {
    return augment_camera<float>(src, dst, B, Hs, Ws, Hd, Wd, C, samples, stream, "augment_camera_f32");
}

extern "C" int dpft_augment_camera_nhwc_u8(const uint8_t* src, float* dst, int32_t B, int32_t Hs, int32_t Ws, int32_t Hd,
                                           int32_t Wd, int32_t C, const dpft_augment_sample* samples,
                                           dpft_stream_t stream) {
    return augment_camera<uint8_t>(src, dst, B, Hs, Ws, Hd, Wd, C, samples, stream, "augment_camera_u8");
}

extern "C" int dpft_augment_radar_nhwc_f32(const float* x, float* y, int32_t B, int32_t H, int32_t W, int32_t C,
                                           int32_t scale, float in_lo, float in_hi, float out_lo, float out_hi,
                                           const dpft_augment_sample* samples, dpft_stream_t stream) {
    DPFT_REQUIRE(x && y && x != y, "augment_radar: null or aliased tensors");
    DPFT_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, "augment_radar: non-positive sizes");
    DPFT_REQUIRE((int64_t)W * C < (1ll << 31), "augment_radar: row too long");
    DPFT_REQUIRE(!scale || in_hi != in_lo, "augment_radar: empty input range");
    DPFT_REQUIRE(samples, "augment_radar: null sample parameters");
    const int64_t n = (int64_t)H * W * C;
    const unsigned gx = (unsigned)std::min<int64_t>(cdiv(n, 256), kNumCU * 16);
    for (int b0 = 0; b0 < B; b0 += DPFT_AUGMENT_CHUNK) {
        const int nb = std::min(DPFT_AUGMENT_CHUNK, B - b0);
        RadarChunk chunk;
        memset(&chunk, 0, sizeof(chunk));
        for (int j = 0; j < nb; ++j) {
            chunk.s[j].delta = samples[b0 + j].delta_db;
            chunk.s[j].flip = samples[b0 + j].flip != 0;
        }
        hipLaunchKernelGGL(augment_radar_kernel, dim3(gx, (unsigned)nb), dim3(256), 0, (hipStream_t)stream, x + b0 * n,
                           y + b0 * n, H, W, C, scale, in_lo, in_hi, out_lo, out_hi, chunk);
        int rc = check_launch("augment_radar");
        if (rc) return rc;
    }
    return DPFT_OK;
}

extern "C" int dpft_augment_geometry_f32(const dpft_augment_view* views, int32_t V, const dpft_augment_labels* labels,
                                         const dpft_augment_sample* samples, int32_t B, dpft_stream_t stream) {
    DPFT_REQUIRE(B > 0 && V >= 0 && V <= DPFT_AUGMENT_MAX_VIEWS && (V == 0 || views), "augment_geometry: bad view table");
    for (int v = 0; v < V; ++v) {
        const dpft_augment_view& w = views[v];
        DPFT_REQUIRE(w.T && w.P && w.T_out && w.P_out && w.shape, "augment_geometry: view %d: null tensor", v);
        DPFT_REQUIRE(w.T != w.T_out && w.P != w.P_out, "augment_geometry: view %d: the outputs must be new tensors", v);
        DPFT_REQUIRE((w.p_rows == 3 || w.p_rows == 4) && w.shape_stride >= 2, "augment_geometry: view %d: P has 3 or 4 rows, "
                     "shape rows hold (H, W, ...)", v);
    }
    int rc = augment_samples_check(samples, B, "augment_geometry");
    if (rc) return rc;
    for (int b = 0; labels && b < B; ++b) {
        const dpft_augment_labels& l = labels[b];
        DPFT_REQUIRE(l.rows >= 0 && (l.rows == 0 || (l.center && l.angle && l.center_out && l.angle_out)),
                     "augment_geometry: sample %d: null label tensor", b);
        DPFT_REQUIRE(l.rows == 0 || (l.center != l.center_out && l.angle != l.angle_out),
                     "augment_geometry: sample %d: the outputs must be new tensors", b);
    }
    for (int b0 = 0; b0 < B; b0 += DPFT_AUGMENT_CHUNK) {
        const int nb = std::min(DPFT_AUGMENT_CHUNK, B - b0);
        GeoTable t;
        memset(&t, 0, sizeof(t));
        for (int v = 0; v < V; ++v) t.view[v] = views[v];
        for (int j = 0; j < nb; ++j) {
            const dpft_augment_sample& a = samples[b0 + j];
            if (labels) t.labels[j] = labels[b0 + j];
            t.s[j] = GeoSample{a.a, a.bu, a.s, a.bv, a.flip != 0, 0};
        }
        t.V = V;
        t.b0 = b0;
        hipLaunchKernelGGL(augment_geometry_kernel, dim3((unsigned)nb), dim3(128), 0, (hipStream_t)stream, t);
        rc = check_launch("augment_geometry");
        if (rc) return rc;
    }
    return DPFT_OK;
}
