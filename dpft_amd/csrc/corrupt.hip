// Sensor degradation on the device (DESIGN.md section 3 "Sensor degradation"): what fog, defocus, sensor noise, a dirty lens or a
// jammed radar sector do to the PREPROCESSED inputs -- the camera frame after its resize (float NHWC, nominally [0, 255]) and
// the scaled radar maps.  Used by the training corruption ("train.corrupt", dpft_amd/data/corrupt.py) and by the robustness
// conditions of the evaluator ("evaluate.robustness", dpft_amd/evaluation/robustness.py).
// The per-sample parameters are fixed on the HOST and travel by value in the kernel arguments, DPFT_CORRUPT_CHUNK samples per
// launch (blockIdx.y = the sample of the chunk).  There is no device random state: the noise is a pure integer function of
// (64-bit key of the sample, view id, element index), restated in tests/corrupt_ref.py.
// This file is compiled with -ffp-contract=off: the point-wise chain rounds operation for operation like that restatement
// (the blur's sums use explicit fmas: one rounding per tap).
#include <math.h>

#include "common.h"

namespace dpft {

constexpr int kTileH = 32, kTileW = 64;      // output pixels of one workgroup; the halo of the blur is R <= DPFT_CORRUPT_MAX_RADIUS around it
constexpr int kRun = 4;                      // outputs, adjacent along the filter's direction, that one thread carries through a pass
constexpr int kTaps = 2 * DPFT_CORRUPT_MAX_RADIUS + 1 + 2 * (kRun - 1);

struct CorruptCam {
    int radius;                                // 0: no blur
    float wp[kTaps];                           // the full table w[|i - R|], i = 0 .. 2R, between kRun - 1 zeros on either side
    float haze, air[4];
    float noise;
    uint32_t s0, s1;                           // the noise stream of (key, view)
    int n_rects;
    int rect[DPFT_CORRUPT_MAX_RECTS][4];       // x0, x1, y0, y1
    float fill[DPFT_CORRUPT_MAX_RECTS][4];
    int off;
};
struct CorruptCamChunk {
    CorruptCam s[DPFT_CORRUPT_CHUNK];
};

// 32-bit multiply-xorshift mixer ("lowbias32")
__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// Irwin-Hall of order 4 out of four 16-bit uniforms of element i: unit variance (exact std 37837.227), |z| < 3.47
__device__ __forceinline__ float noise_z(uint32_t s0, uint32_t s1, uint32_t i) {
    const uint32_t a = mix32(i ^ s0), b = mix32(a ^ s1);
    const int sum = (int)((a & 0xffffu) + (a >> 16) + (b & 0xffffu) + (b >> 16)) - 131070;
    return (float)sum * (1.0f / 37837.2f);
}

static void noise_stream(uint64_t key, int32_t view, uint32_t* s0, uint32_t* s1) {
    const uint32_t lo = (uint32_t)key, hi = (uint32_t)(key >> 32), v = (uint32_t)view;
    *s0 = mix32(lo ^ mix32(hi ^ mix32(v ^ 0x9e3779b9u)));
    *s1 = mix32(hi ^ mix32(lo ^ mix32(v ^ 0xc2b2ae35u)));
}

__device__ __forceinline__ float clamp_range(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// haze -> noise -> erase of element (x, y, c) of the frame; `i` = (y W + x) C + c
__device__ __forceinline__ float camera_chain(const CorruptCam& p, float v, int x, int y, int c, uint32_t i) {
    if (p.haze != 0.f) {
        const float d = p.air[c] - v;
        const float t = p.haze * d;
        v = v + t;
    }
    if (p.noise > 0.f) {
        const float t = p.noise * noise_z(p.s0, p.s1, i);
        v = clamp_range(v + t, 0.f, 255.f);
    }
    for (int j = 0; j < p.n_rects; ++j)
        if (x >= p.rect[j][0] && x < p.rect[j][1] && y >= p.rect[j][2] && y < p.rect[j][3]) v = p.fill[j][c];
    return v;
}

// One workgroup per kTileH x kTileW tile of one sample.  A blurred sample stages the tile and its halo of R pixels (replicate
// border) in LDS once, runs the horizontal pass LDS -> LDS over the tile's rows and the halo rows above and below, and the
// vertical pass LDS -> registers, then the point-wise chain and the store.  Rows are handled as runs of (pixels * C) floats:
// in the staging loop, the vertical pass and the stores consecutive threads touch consecutive LDS words and consecutive global
// floats (in the horizontal pass a thread owns kRun pixels of one channel, its neighbours the other channels and the next pixels).
// Dynamic LDS: ((kTileH + 2 Rmax) (kTileW + 2 Rmax) + (kTileH + 2 Rmax) kTileW) C floats, Rmax = the launch's largest radius.
__global__ __launch_bounds__(256) void corrupt_camera_kernel(const float* __restrict__ src, float* __restrict__ dst, int H,
                                                              int W, int C, int tiles_x, const CorruptCamChunk chunk) {
    extern __shared__ float lds[];
    const CorruptCam& p = chunk.s[blockIdx.y];
    const float* frame = src + (int64_t)blockIdx.y * H * W * C;
    float* out = dst + (int64_t)blockIdx.y * H * W * C;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * kTileH, x0 = tx * kTileW;
    const int th = min(kTileH, H - y0), tw = min(kTileW, W - x0);
    const int run = tw * C, n = th * run;
    const int R = p.radius;
    if (p.off) {
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int r = i / run, rem = i - r * run;
            out[((int64_t)(y0 + r) * W + x0) * C + rem] = 0.f;
        }
        return;
    }
    if (R == 0) {
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int r = i / run, rem = i - r * run;
            const int x = rem / C, c = rem - x * C;
            const int64_t g = ((int64_t)(y0 + r) * W + x0) * C + rem;
            out[g] = camera_chain(p, frame[g], x0 + x, y0 + r, c, (uint32_t)g);
        }
        return;
    }
    const int sh = th + 2 * R, sw = tw + 2 * R, srun = sw * C;
    float* in = lds;
    float* mid = lds + sh * srun;
    for (int i = threadIdx.x; i < sh * srun; i += blockDim.x) {
        const int r = i / srun, rem = i - r * srun;
        const int xx = rem / C, c = rem - xx * C;
        const int gy = min(max(y0 - R + r, 0), H - 1), gx = min(max(x0 - R + xx, 0), W - 1);
        in[i] = frame[((int64_t)gy * W + gx) * C + c];
    }
    __syncthreads();
    // Every thread carries kRun adjacent outputs through a pass: one LDS read feeds up to kRun sums (kRun + 2R reads for kRun
    // outputs instead of kRun (2R + 1)) and the sums are independent chains.  The zeros around the table make the edge taps of
    // the run plain fmas with weight 0 (no branches); a read past the staged block is clamped, it only feeds such a zero tap
    // or an output beyond the tile that is not stored.
    const int nin = kRun + 2 * R;
    const int groups = (tw + kRun - 1) / kRun, gc = groups * C;
    for (int i = threadIdx.x; i < sh * gc; i += blockDim.x) {
        const int r = i / gc, rem = i - r * gc;
        const int g = rem / C, c = rem - g * C;
        const float* q = in + r * srun + c;
        float acc[kRun] = {};
        for (int j = 0; j < nin; ++j) {
            const float v = q[min(g * kRun + j, sw - 1) * C];
#pragma unroll
            for (int o = 0; o < kRun; ++o) acc[o] = __builtin_fmaf(p.wp[j - o + kRun - 1], v, acc[o]);
        }
#pragma unroll
        for (int o = 0; o < kRun; ++o)
            if (g * kRun + o < tw) mid[r * run + (g * kRun + o) * C + c] = acc[o];
    }
    __syncthreads();
    const int segs = (th + kRun - 1) / kRun;
    for (int i = threadIdx.x; i < segs * run; i += blockDim.x) {
        const int seg = i / run, rem = i - seg * run;
        const int r0 = seg * kRun;
        float acc[kRun] = {};
        for (int j = 0; j < nin; ++j) {
            const float v = mid[min(r0 + j, sh - 1) * run + rem];
#pragma unroll
            for (int o = 0; o < kRun; ++o) acc[o] = __builtin_fmaf(p.wp[j - o + kRun - 1], v, acc[o]);
        }
        const int x = rem / C, c = rem - x * C;
#pragma unroll
        for (int o = 0; o < kRun; ++o) {
            const int r = r0 + o;
            if (r < th) {
                const int64_t gi = ((int64_t)(y0 + r) * W + x0) * C + rem;
                out[gi] = camera_chain(p, acc[o], x0 + x, y0 + r, c, (uint32_t)gi);
            }
        }
    }
}

struct CorruptRad {
    float noise;
    uint32_t s0, s1, channels;
    int n_az, n_rows;
    int az[DPFT_CORRUPT_MAX_BANDS][2], rows[DPFT_CORRUPT_MAX_BANDS][2];
    int off;
};
struct CorruptRadChunk {
    CorruptRad s[DPFT_CORRUPT_CHUNK];
};

// One thread per element of (H, W, C): noise on the selected channels, azimuth (axis 2 of (B,H,W,C)) and row bands to `lo`, off to 0
__global__ __launch_bounds__(256) void corrupt_radar_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W,
                                                             int C, float lo, float hi, const CorruptRadChunk chunk) {
    const CorruptRad& p = chunk.s[blockIdx.y];
    const int n = H * W * C, wc = W * C;
    const float* xs = x + (int64_t)blockIdx.y * n;
    float* ys = y + (int64_t)blockIdx.y * n;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (p.off) {
            ys[i] = 0.f;
            continue;
        }
        const int r = i / wc, rem = i - r * wc;
        const int a = rem / C, c = rem - a * C;
        float v = xs[i];
        if (p.noise > 0.f && ((p.channels >> c) & 1u)) {
            const float t = p.noise * noise_z(p.s0, p.s1, (uint32_t)i);
            v = clamp_range(v + t, lo, hi);
        }
        for (int j = 0; j < p.n_az; ++j)
            if (a >= p.az[j][0] && a < p.az[j][1]) v = lo;
        for (int j = 0; j < p.n_rows; ++j)
            if (r >= p.rows[j][0] && r < p.rows[j][1]) v = lo;
        ys[i] = v;
    }
}

static bool finite_in(float v, float lo, float hi) { return v >= lo && v <= hi; }      // (false for NaN)

static int corrupt_camera_check(const dpft_corrupt_camera& a, int b, int H, int W) {
    const char* what = "corrupt_camera";
    DPFT_REQUIRE(finite_in(a.sigma, 0.f, 5.f), "%s: sample %d: sigma must lie in [0, 5]", what, b);
    DPFT_REQUIRE(a.radius >= 0 && a.radius <= DPFT_CORRUPT_MAX_RADIUS && (a.radius > 0) == (a.sigma > 0.f),
                 "%s: sample %d: radius must be ceil(3 sigma) in 0..%d, 0 exactly when sigma is 0 (got %d)", what, b,
                 DPFT_CORRUPT_MAX_RADIUS, a.radius);
    if (a.radius > 0) {
        double sum = 0.0;
        for (int k = 0; k <= a.radius; ++k) {
            DPFT_REQUIRE(finite_in(a.w[k], 0.f, 1.f), "%s: sample %d: weight %d outside [0, 1]", what, b, k);
            sum += (k ? 2.0 : 1.0) * (double)a.w[k];
        }
        DPFT_REQUIRE(fabs(sum - 1.0) <= 1e-5, "%s: sample %d: the weights w[0] + 2 sum w[k] must add up to 1 (got %.9g)", what,
                     b, sum);
    }
    DPFT_REQUIRE(finite_in(a.haze, 0.f, 1.f), "%s: sample %d: haze must lie in [0, 1]", what, b);
    for (int c = 0; c < 4; ++c)
        DPFT_REQUIRE(finite_in(a.airlight[c], 0.f, 255.f), "%s: sample %d: airlight must lie in [0, 255]", what, b);
    DPFT_REQUIRE(finite_in(a.noise, 0.f, 3.0e38f), "%s: sample %d: noise must be finite and >= 0", what, b);
    DPFT_REQUIRE(a.n_rects >= 0 && a.n_rects <= DPFT_CORRUPT_MAX_RECTS, "%s: sample %d: at most %d rectangles", what, b,
                 DPFT_CORRUPT_MAX_RECTS);
    for (int j = 0; j < a.n_rects; ++j) {
        const int32_t* r = a.rect[j];
        DPFT_REQUIRE(0 <= r[0] && r[0] <= r[1] && r[1] <= W && 0 <= r[2] && r[2] <= r[3] && r[3] <= H,
                     "%s: sample %d: rectangle %d [%d, %d) x [%d, %d) leaves the %d x %d frame", what, b, j, r[0], r[1], r[2],
                     r[3], W, H);
        for (int c = 0; c < 4; ++c)
            DPFT_REQUIRE(finite_in(a.fill[j][c], -3.0e38f, 3.0e38f), "%s: sample %d: rectangle %d: fill not finite", what, b, j);
    }
    return DPFT_OK;
}

static int corrupt_bands_check(const int32_t (*band)[2], int n, int size, int b, const char* axis) {
    DPFT_REQUIRE(n >= 0 && n <= DPFT_CORRUPT_MAX_BANDS, "corrupt_radar: sample %d: at most %d %s bands", b,
                 DPFT_CORRUPT_MAX_BANDS, axis);
    for (int j = 0; j < n; ++j)
        DPFT_REQUIRE(0 <= band[j][0] && band[j][0] <= band[j][1] && band[j][1] <= size,
                     "corrupt_radar: sample %d: %s band %d [%d, %d) leaves the axis of %d", b, axis, j, band[j][0], band[j][1],
                     size);
    return DPFT_OK;
}

}  // namespace dpft

using namespace dpft;

extern "C" int dpft_corrupt_limits(int32_t out[4]) {
    DPFT_REQUIRE(out, "corrupt_limits: null output");
    out[0] = kTileH; out[1] = kTileW; out[2] = DPFT_CORRUPT_MAX_RADIUS; out[3] = DPFT_CORRUPT_CHUNK;
    return DPFT_OK;
}

extern "C" int dpft_corrupt_camera_nhwc_f32(const float* src, float* dst, int32_t B, int32_t H, int32_t W, int32_t C,
                                            const dpft_corrupt_camera* samples, dpft_stream_t stream) {
    DPFT_REQUIRE(src && dst && src != dst, "corrupt_camera: null or aliased tensors");
    DPFT_REQUIRE(samples, "corrupt_camera: null sample parameters");
    DPFT_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, "corrupt_camera: non-positive sizes");
    DPFT_REQUIRE(C <= 4, "corrupt_camera: at most 4 channels (got %d)", C);
    DPFT_REQUIRE((int64_t)H * W < (1ll << 29), "corrupt_camera: frame too large");
    for (int b = 0; b < B; ++b) {
        int rc = corrupt_camera_check(samples[b], b, H, W);
        if (rc) return rc;
    }
    const int tiles_x = cdiv(W, kTileW), tiles = tiles_x * cdiv(H, kTileH);
    static LdsGrant grant;
    for (int b0 = 0; b0 < B; b0 += DPFT_CORRUPT_CHUNK) {
        const int nb = std::min(DPFT_CORRUPT_CHUNK, B - b0);
        CorruptCamChunk chunk;
        memset(&chunk, 0, sizeof(chunk));
        int rmax = 0;
        for (int j = 0; j < nb; ++j) {
            const dpft_corrupt_camera& a = samples[b0 + j];
            CorruptCam& c = chunk.s[j];
            c.radius = a.radius;
            for (int k = 0; k <= 2 * a.radius && a.radius > 0; ++k) c.wp[kRun - 1 + k] = a.w[abs(k - a.radius)];
            c.haze = a.haze;
            for (int k = 0; k < 4; ++k) c.air[k] = a.airlight[k];
            c.noise = a.noise;
            noise_stream(a.key, a.view, &c.s0, &c.s1);
            c.n_rects = a.n_rects;
            for (int r = 0; r < a.n_rects; ++r)
                for (int k = 0; k < 4; ++k) {
                    c.rect[r][k] = a.rect[r][k];
                    c.fill[r][k] = a.fill[r][k];
                }
            c.off = a.off != 0;
            if (!c.off) rmax = std::max(rmax, c.radius);
            else c.radius = 0;
        }
        const size_t lds = rmax ? (size_t)(kTileH + 2 * rmax) * ((kTileW + 2 * rmax) + kTileW) * C * sizeof(float) : 0;
        DPFT_REQUIRE(lds_grant(grant, (const void*)corrupt_camera_kernel, lds), "corrupt_camera: %zu bytes of LDS refused", lds);
        hipLaunchKernelGGL(corrupt_camera_kernel, dim3((unsigned)tiles, (unsigned)nb), dim3(256), lds, (hipStream_t)stream,
                           src + (int64_t)b0 * H * W * C, dst + (int64_t)b0 * H * W * C, H, W, C, tiles_x, chunk);
        int rc = check_launch("corrupt_camera");
        if (rc) return rc;
    }
    return DPFT_OK;
}

extern "C" int dpft_corrupt_radar_nhwc_f32(const float* x, float* y, int32_t B, int32_t H, int32_t W, int32_t C, float lo,
                                           float hi, const dpft_corrupt_radar* samples, dpft_stream_t stream) {
    DPFT_REQUIRE(x && y && x != y, "corrupt_radar: null or aliased tensors");
    DPFT_REQUIRE(samples, "corrupt_radar: null sample parameters");
    DPFT_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, "corrupt_radar: non-positive sizes");
    DPFT_REQUIRE(C <= 32, "corrupt_radar: at most 32 channels (the channel mask has 32 bits; got %d)", C);
    DPFT_REQUIRE((int64_t)H * W * C < (1ll << 31), "corrupt_radar: map too large");
    DPFT_REQUIRE(lo <= hi && finite_in(lo, -3.0e38f, 3.0e38f) && finite_in(hi, -3.0e38f, 3.0e38f),
                 "corrupt_radar: the range [lo, hi] must be finite and ordered");
    for (int b = 0; b < B; ++b) {
        const dpft_corrupt_radar& a = samples[b];
        DPFT_REQUIRE(finite_in(a.noise, 0.f, 3.0e38f), "corrupt_radar: sample %d: noise must be finite and >= 0", b);
        int rc = corrupt_bands_check(a.azimuth, a.n_azimuth, W, b, "azimuth");
        if (rc) return rc;
        rc = corrupt_bands_check(a.rows, a.n_rows, H, b, "row");
        if (rc) return rc;
    }
    const int n = H * W * C;
    const unsigned gx = (unsigned)std::min<int64_t>(cdiv(n, 256), kNumCU * 16);
    for (int b0 = 0; b0 < B; b0 += DPFT_CORRUPT_CHUNK) {
        const int nb = std::min(DPFT_CORRUPT_CHUNK, B - b0);
        CorruptRadChunk chunk;
        memset(&chunk, 0, sizeof(chunk));
        for (int j = 0; j < nb; ++j) {
            const dpft_corrupt_radar& a = samples[b0 + j];
            CorruptRad& c = chunk.s[j];
            c.noise = a.noise;
            c.channels = a.channels;
            noise_stream(a.key, a.view, &c.s0, &c.s1);
            c.n_az = a.n_azimuth;
            c.n_rows = a.n_rows;
            for (int k = 0; k < a.n_azimuth; ++k) { c.az[k][0] = a.azimuth[k][0]; c.az[k][1] = a.azimuth[k][1]; }
            for (int k = 0; k < a.n_rows; ++k) { c.rows[k][0] = a.rows[k][0]; c.rows[k][1] = a.rows[k][1]; }
            c.off = a.off != 0;
        }
        hipLaunchKernelGGL(corrupt_radar_kernel, dim3(gx, (unsigned)nb), dim3(256), 0, (hipStream_t)stream,
                           x + (int64_t)b0 * n, y + (int64_t)b0 * n, H, W, C, lo, hi, chunk);
        int rc = check_launch("corrupt_radar");
        if (rc) return rc;
    }
    return DPFT_OK;
}
