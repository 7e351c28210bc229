// Multi-scale deformable attention operator with typed storage for gfx950: dpft_msda_{fwd,bwd}_typed.
//
// Same operator as msda.hip (1) -- value (N,S,M,D), shapes (L,2) int64 rows (H,W), lsi (L) int64, loc (N,Lq,M,L,P,2) as (x,y),
// attn (N,Lq,M,L,P), out (N,Lq,M*D) -- and the project's one sampling rule: t = loc * size - 0.5, a sample
// counts iff -1 < t < size on both axes, the four corners are bounds-checked one by one.  The bilinear variable names (h_im /
// w_im, lh / lw / hh / hw, v1..v4) are those of msda.hip (attribution there).
//
// Storage type T in {float, IEEE half, bf16}; `loc` / `grad_loc` either T or fp32 (what autocast hands over).  All arithmetic
// is fp32, operands are upcast exactly on load, and every result is rounded to its storage type exactly once, to nearest even.
// The file is compiled with -ffp-contract=off (Makefile): the vector and the scalar forward then run the same IEEE operations
// in the same order per channel, so which of the two an alignment selects does not change a bit of the result.
//
// Forward, vector form: a lane owns 16 bytes of one head (8 channels of 16-bit storage, 4 of fp32): one 16-byte load per
//   corner, loc / attn once per (head, level, point) and lane, one 16-byte store.  A wave takes as many whole queries as fit
//   (2 at M * D = 256 in 16-bit storage); a query wider than a wave takes whole waves.  Needs D % 8 == 0 (D % 4 for fp32) and
//   16-byte aligned value / out; everything else takes the scalar form (one lane per output channel).
// Backward: lane = channel.  A head owns a group of G = min(64, next power of two >= D) lanes (lanes beyond D idle, D > 64
//   loops), 64 / G heads per wave.  grad_attn / grad_loc: partials over the head's channels summed inside the wave by
//   xor-shuffles over the group, stored by its first lane (grad_loc scaled by W / H before its one rounding).  grad_value: fp32
//   atomics into an fp32 workspace, one dword per lane, a group's lanes on consecutive channels of one pixel row -- at D = 32
//   a wave-instruction is two 128-byte row segments, at D >= 64 one 256-byte run, the two shapes MI355X adds at its full
//   atomic rate -- then one convert pass rounds the sums to T (fp32: the workspace is grad_value itself, no pass).
//   Packed 16-bit atomics are not used: they would round the running sum at every add.
// No allocation, no synchronisation, kernel nodes only (the workspace is cleared by a kernel): capturable in a hipGraph.
#include <algorithm>

#include "common.h"

namespace dpft {
namespace {

struct bf16_t {
    unsigned short u;
};

template <typename T> struct Storage;
template <> struct Storage<float> {
    static constexpr int VEC = 4;
    static __device__ __forceinline__ float up(float v) { return v; }
    static __device__ __forceinline__ float down(float f) { return f; }
};
template <> struct Storage<_Float16> {
    static constexpr int VEC = 8;
    static __device__ __forceinline__ float up(_Float16 v) { return (float)v; }
    static __device__ __forceinline__ _Float16 down(float f) { return (_Float16)f; }      // v_cvt_f16_f32: nearest even
};
template <> struct Storage<bf16_t> {
    static constexpr int VEC = 8;
    static __device__ __forceinline__ float up(bf16_t v) { return __uint_as_float((unsigned)v.u << 16); }
    static __device__ __forceinline__ bf16_t down(float f) {
        const unsigned u = __float_as_uint(f);
        if ((u & 0x7fffffffu) > 0x7f800000u) return bf16_t{(unsigned short)((u >> 16) | 0x40u)};      // NaN stays NaN
        return bf16_t{(unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16)};                        // nearest even
    }
};

template <typename T> struct alignas(16) Pack {
    T v[Storage<T>::VEC];
};

// the bilinear cell of one sample: which corners count, their weights and their pixel offsets (in pixels, not elements)
struct Cell {
    bool in, k1, k2, k3, k4;
    float lh, lw, hh, hw;
    int64_t p1, p2, p3, p4;
};
__device__ __forceinline__ Cell cell_of(float lx, float ly, int H, int W) {
    Cell c;
    const float h_im = ly * H - 0.5f, w_im = lx * W - 0.5f;
    c.in = h_im > -1 && w_im > -1 && h_im < H && w_im < W;
    c.k1 = c.k2 = c.k3 = c.k4 = false;
    c.lh = c.lw = c.hh = c.hw = 0.f;
    c.p1 = c.p2 = c.p3 = c.p4 = 0;
    if (c.in) {
        const int h_lo = (int)floorf(h_im), w_lo = (int)floorf(w_im);
        const int h_hi = h_lo + 1, w_hi = w_lo + 1;
        c.lh = h_im - h_lo; c.lw = w_im - w_lo; c.hh = 1 - c.lh; c.hw = 1 - c.lw;
        c.k1 = h_lo >= 0 && w_lo >= 0; c.k2 = h_lo >= 0 && w_hi <= W - 1;
        c.k3 = h_hi <= H - 1 && w_lo >= 0; c.k4 = h_hi <= H - 1 && w_hi <= W - 1;
        c.p1 = (int64_t)h_lo * W + w_lo; c.p2 = (int64_t)h_lo * W + w_hi;
        c.p3 = (int64_t)h_hi * W + w_lo; c.p4 = (int64_t)h_hi * W + w_hi;
    }
    return c;
}
// one channel's share of one sample: the single expression both forward forms evaluate
__device__ __forceinline__ float tap(const Cell& c, float a, float v1, float v2, float v3, float v4) {
    return a * (c.hh * c.hw * v1 + c.hh * c.lw * v2 + c.lh * c.hw * v3 + c.lh * c.lw * v4);
}

// ---------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------
// qpw > 0: a wave takes qpw whole queries of lpq lanes each (the lanes beyond qpw * lpq idle); qpw == 0: a query takes wpq whole waves
template <typename T, typename TL>
__global__ __launch_bounds__(256) void msda_fwd_vec_kernel(const T* __restrict__ value, const int64_t* __restrict__ shapes,
                                                            const int64_t* __restrict__ lsi, const TL* __restrict__ loc,
                                                            const T* __restrict__ attn, T* __restrict__ out, int N, int S,
                                                            int M, int D, int Lq, int L, int P, int lpq, int qpw, int wpq) {
    constexpr int VEC = Storage<T>::VEC;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t NQ = (int64_t)N * Lq;
    int64_t bq;
    int j;
    if (qpw > 0) {
        const int qi = lane / lpq;
        if (qi >= qpw) return;
        bq = wave * qpw + qi;
        j = lane - qi * lpq;
    } else {
        bq = wave / wpq;
        j = (int)(wave % wpq) * 64 + lane;
        if (j >= lpq) return;
    }
    if (bq >= NQ) return;
    const int b = (int)(bq / Lq);
    const int ch = j * VEC;            // first of this lane's channels in the query's M * D
    const int m = ch / D;
    const int64_t rs = (int64_t)M * D;
    const int64_t lp = (bq * M + m) * L * P;
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    for (int l = 0; l < L; ++l) {
        const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
        const T* base = value + ((int64_t)b * S + lsi[l]) * rs + ch;
        for (int p = 0; p < P; ++p) {
            const float lx = Storage<TL>::up(loc[(lp + l * P + p) * 2 + 0]), ly = Storage<TL>::up(loc[(lp + l * P + p) * 2 + 1]);
            const float a = Storage<T>::up(attn[lp + l * P + p]);
            const Cell c = cell_of(lx, ly, H, W);
            if (c.in) {
                Pack<T> v1 = {}, v2 = {}, v3 = {}, v4 = {};
                if (c.k1) v1 = *reinterpret_cast<const Pack<T>*>(base + c.p1 * rs);
                if (c.k2) v2 = *reinterpret_cast<const Pack<T>*>(base + c.p2 * rs);
                if (c.k3) v3 = *reinterpret_cast<const Pack<T>*>(base + c.p3 * rs);
                if (c.k4) v4 = *reinterpret_cast<const Pack<T>*>(base + c.p4 * rs);
#pragma unroll
                for (int e = 0; e < VEC; ++e)
                    acc[e] += tap(c, a, Storage<T>::up(v1.v[e]), Storage<T>::up(v2.v[e]), Storage<T>::up(v3.v[e]),
                                  Storage<T>::up(v4.v[e]));
            }
        }
    }
    Pack<T> o;
#pragma unroll
    for (int e = 0; e < VEC; ++e) o.v[e] = Storage<T>::down(acc[e]);
    *reinterpret_cast<Pack<T>*>(out + bq * rs + ch) = o;
}

template <typename T, typename TL>
__global__ __launch_bounds__(256) void msda_fwd_scalar_kernel(const T* __restrict__ value, const int64_t* __restrict__ shapes,
                                                               const int64_t* __restrict__ lsi, const TL* __restrict__ loc,
                                                               const T* __restrict__ attn, T* __restrict__ out, int N, int S,
                                                               int M, int D, int Lq, int L, int P) {
    const int64_t rs = (int64_t)M * D;
    const int64_t total = (int64_t)N * Lq * rs;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int64_t bq = idx / rs;
    const int ch = (int)(idx - bq * rs);
    const int m = ch / D;
    const int b = (int)(bq / Lq);
    const int64_t lp = (bq * M + m) * L * P;
    float acc = 0.f;
    for (int l = 0; l < L; ++l) {
        const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
        const T* base = value + ((int64_t)b * S + lsi[l]) * rs + ch;
        for (int p = 0; p < P; ++p) {
            const float lx = Storage<TL>::up(loc[(lp + l * P + p) * 2 + 0]), ly = Storage<TL>::up(loc[(lp + l * P + p) * 2 + 1]);
            const float a = Storage<T>::up(attn[lp + l * P + p]);
            const Cell c = cell_of(lx, ly, H, W);
            if (c.in) {
                const float v1 = c.k1 ? Storage<T>::up(base[c.p1 * rs]) : 0.f, v2 = c.k2 ? Storage<T>::up(base[c.p2 * rs]) : 0.f;
                const float v3 = c.k3 ? Storage<T>::up(base[c.p3 * rs]) : 0.f, v4 = c.k4 ? Storage<T>::up(base[c.p4 * rs]) : 0.f;
                acc += tap(c, a, v1, v2, v3, v4);
            }
        }
    }
    out[idx] = Storage<T>::down(acc);
}

// ---------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------
// gs = log2(G): a head's lane group; the lanes of a group run the same (level, point) loop, so the shuffles below never read a
// lane that has left it (a group past the end of the work keeps running on the last head with every store and atomic masked)
template <typename T, typename TL>
__global__ __launch_bounds__(256) void msda_bwd_kernel_typed(const T* __restrict__ value, const int64_t* __restrict__ shapes,
                                                              const int64_t* __restrict__ lsi, const TL* __restrict__ loc,
                                                              const T* __restrict__ attn, const T* __restrict__ gout,
                                                              float* __restrict__ gvalue32, TL* __restrict__ gloc,
                                                              T* __restrict__ gattn, int N, int S, int M, int D, int Lq, int L,
                                                              int P, int gs) {
    const int lane = threadIdx.x & 63;
    const int G = 1 << gs;
    const int g = lane & (G - 1);
    const int64_t heads = (int64_t)N * Lq * M;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    int64_t item = (wave << (6 - gs)) + (lane >> gs);
    const bool live = item < heads;
    if (!live) item = heads - 1;
    const int m = (int)(item % M);
    const int b = (int)(item / ((int64_t)M * Lq));
    const int64_t rs = (int64_t)M * D;
    const int64_t lp = item * L * P;
    const T* go = gout + item * D;
    for (int l = 0; l < L; ++l) {
        const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
        const int64_t boff = ((int64_t)b * S + lsi[l]) * rs + (int64_t)m * D;
        for (int p = 0; p < P; ++p) {
            const float lx = Storage<TL>::up(loc[(lp + l * P + p) * 2 + 0]), ly = Storage<TL>::up(loc[(lp + l * P + p) * 2 + 1]);
            const float a = Storage<T>::up(attn[lp + l * P + p]);
            const Cell c = cell_of(lx, ly, H, W);
            float ga = 0.f, gw = 0.f, gh = 0.f;
            if (c.in && live) {
                const int64_t o1 = boff + c.p1 * rs, o2 = boff + c.p2 * rs, o3 = boff + c.p3 * rs, o4 = boff + c.p4 * rs;
                const float w1 = c.hh * c.hw, w2 = c.hh * c.lw, w3 = c.lh * c.hw, w4 = c.lh * c.lw;
                for (int ch = g; ch < D; ch += G) {
                    const float gr = Storage<T>::up(go[ch]), tg = gr * a;
                    const float v1 = c.k1 ? Storage<T>::up(value[o1 + ch]) : 0.f, v2 = c.k2 ? Storage<T>::up(value[o2 + ch]) : 0.f;
                    const float v3 = c.k3 ? Storage<T>::up(value[o3 + ch]) : 0.f, v4 = c.k4 ? Storage<T>::up(value[o4 + ch]) : 0.f;
                    if (c.k1) atomicAdd(gvalue32 + o1 + ch, w1 * tg);
                    if (c.k2) atomicAdd(gvalue32 + o2 + ch, w2 * tg);
                    if (c.k3) atomicAdd(gvalue32 + o3 + ch, w3 * tg);
                    if (c.k4) atomicAdd(gvalue32 + o4 + ch, w4 * tg);
                    ga += gr * (w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4);
                    gh += tg * (-c.hw * v1 - c.lw * v2 + c.hw * v3 + c.lw * v4);
                    gw += tg * (-c.hh * v1 + c.hh * v2 - c.lh * v3 + c.lh * v4);
                }
            }
            for (int o = 1; o < G; o <<= 1) {
                ga += __shfl_xor(ga, o);
                gw += __shfl_xor(gw, o);
                gh += __shfl_xor(gh, o);
            }
            if (g == 0 && live) {
                gattn[lp + l * P + p] = Storage<T>::down(ga);
                gloc[(lp + l * P + p) * 2 + 0] = Storage<TL>::down(W * gw);
                gloc[(lp + l * P + p) * 2 + 1] = Storage<TL>::down(H * gh);
            }
        }
    }
}

// fp32 sums -> T, rounded once; 8 elements per lane with 16-byte accesses where `dst` allows, element by element otherwise
template <typename T>
__global__ __launch_bounds__(256) void msda_round_kernel(const float* __restrict__ src, T* __restrict__ dst, int64_t n, int vec) {
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i0 >= n) return;
    if (vec && i0 + 8 <= n) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(src + i0), b = *reinterpret_cast<const f32x4*>(src + i0 + 4);
        Pack<T> o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o.v[e] = Storage<T>::down(a[e]);
            o.v[4 + e] = Storage<T>::down(b[e]);
        }
        *reinterpret_cast<Pack<T>*>(dst + i0) = o;
    } else {
        for (int64_t i = i0; i < n && i < i0 + 8; ++i) dst[i] = Storage<T>::down(src[i]);
    }
}

__global__ __launch_bounds__(256) void msda_clear_kernel(float* __restrict__ p, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) p[i] = 0.f;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct Dims {
    int N, S, M, D, Lq, L, P;
};

template <typename T, typename TL>
int launch_fwd(const void* value, const int64_t* shapes, const int64_t* lsi, const void* loc, const void* attn, void* out,
               const Dims& d, hipStream_t st) {
    constexpr int VEC = Storage<T>::VEC;
    const int64_t NQ = (int64_t)d.N * d.Lq, rs = (int64_t)d.M * d.D;
    if (d.D % VEC == 0 && aligned16(value) && aligned16(out)) {
        const int lpq = (int)(rs / VEC);
        const int qpw = lpq <= 64 ? 64 / lpq : 0, wpq = lpq <= 64 ? 1 : cdiv(lpq, 64);
        const int64_t waves = qpw ? (NQ + qpw - 1) / qpw : NQ * wpq;
        hipLaunchKernelGGL((msda_fwd_vec_kernel<T, TL>), dim3(cdiv(waves, 4)), dim3(256), 0, st, (const T*)value, shapes, lsi,
                           (const TL*)loc, (const T*)attn, (T*)out, d.N, d.S, d.M, d.D, d.Lq, d.L, d.P, lpq, qpw, wpq);
    } else {
        hipLaunchKernelGGL((msda_fwd_scalar_kernel<T, TL>), dim3(cdiv(NQ * rs, 256)), dim3(256), 0, st, (const T*)value, shapes,
                           lsi, (const TL*)loc, (const T*)attn, (T*)out, d.N, d.S, d.M, d.D, d.Lq, d.L, d.P);
    }
    return check_launch("msda_fwd_typed");
}

template <typename T, typename TL>
int launch_bwd(const void* value, const int64_t* shapes, const int64_t* lsi, const void* loc, const void* attn,
               const void* grad_out, void* grad_value, void* grad_loc, void* grad_attn, float* sums, const Dims& d,
               dpft_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)d.N * d.S * d.M * d.D;
    if (aligned16(sums)) {
        const int rc = zero_fill(sums, (size_t)n * 4, stream);
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL(msda_clear_kernel, dim3((int)std::min<int64_t>(kNumCU * 8, (n + 255) / 256)), dim3(256), 0, st, sums, n);
        const int rc = check_launch("msda_bwd_typed");
        if (rc) return rc;
    }
    int gs = 0;
    while (gs < 6 && (1 << gs) < d.D) ++gs;
    const int64_t heads = (int64_t)d.N * d.Lq * d.M;
    const int64_t waves = (heads + (64 >> gs) - 1) >> (6 - gs);
    hipLaunchKernelGGL((msda_bwd_kernel_typed<T, TL>), dim3(cdiv(waves, 4)), dim3(256), 0, st, (const T*)value, shapes, lsi,
                       (const TL*)loc, (const T*)attn, (const T*)grad_out, sums, (TL*)grad_loc, (T*)grad_attn, d.N, d.S, d.M,
                       d.D, d.Lq, d.L, d.P, gs);
    int rc = check_launch("msda_bwd_typed");
    if (rc) return rc;
    if ((void*)sums != grad_value) {
        hipLaunchKernelGGL((msda_round_kernel<T>), dim3(cdiv(n, 2048)), dim3(256), 0, st, sums, (T*)grad_value, n,
                           (int)(aligned16(sums) && aligned16(grad_value)));
        rc = check_launch("msda_bwd_typed");
    }
    return rc;
}

}  // namespace
}  // namespace dpft

using namespace dpft;

extern "C" int dpft_msda_fwd_typed(const void* value, const int64_t* shapes, const int64_t* lsi, const void* loc,
                                   const void* attn, void* out, int32_t N, int32_t S, int32_t M, int32_t D, int32_t Lq,
                                   int32_t L, int32_t P, int32_t dtype, int32_t loc32, dpft_stream_t stream) {
    DPFT_REQUIRE(value && shapes && lsi && loc && attn && out, "msda_fwd_typed: null tensor");
    DPFT_REQUIRE(N > 0 && S > 0 && M > 0 && D > 0 && Lq > 0 && L > 0 && P > 0, "msda_fwd_typed: non-positive dims");
    DPFT_REQUIRE(dtype >= 0 && dtype <= 2, "msda_fwd_typed: dtype %d (0 fp32 | 1 half | 2 bf16)", dtype);
    DPFT_REQUIRE(loc32 == 0 || loc32 == 1, "msda_fwd_typed: loc32 %d (0 | 1)", loc32);
    const Dims d{N, S, M, D, Lq, L, P};
    hipStream_t st = (hipStream_t)stream;
    if (dtype == 0) return launch_fwd<float, float>(value, shapes, lsi, loc, attn, out, d, st);
    if (dtype == 1)
        return loc32 ? launch_fwd<_Float16, float>(value, shapes, lsi, loc, attn, out, d, st)
                     : launch_fwd<_Float16, _Float16>(value, shapes, lsi, loc, attn, out, d, st);
    return loc32 ? launch_fwd<bf16_t, float>(value, shapes, lsi, loc, attn, out, d, st)
                 : launch_fwd<bf16_t, bf16_t>(value, shapes, lsi, loc, attn, out, d, st);
}

extern "C" int dpft_msda_bwd_typed(const void* value, const int64_t* shapes, const int64_t* lsi, const void* loc,
                                   const void* attn, const void* grad_out, void* grad_value, void* grad_loc, void* grad_attn,
                                   float* workspace, int32_t N, int32_t S, int32_t M, int32_t D, int32_t Lq, int32_t L,
                                   int32_t P, int32_t dtype, int32_t loc32, dpft_stream_t stream) {
    DPFT_REQUIRE(value && shapes && lsi && loc && attn && grad_out && grad_value && grad_loc && grad_attn,
                 "msda_bwd_typed: null tensor");
    DPFT_REQUIRE(N > 0 && S > 0 && M > 0 && D > 0 && Lq > 0 && L > 0 && P > 0, "msda_bwd_typed: non-positive dims");
    DPFT_REQUIRE(dtype >= 0 && dtype <= 2, "msda_bwd_typed: dtype %d (0 fp32 | 1 half | 2 bf16)", dtype);
    DPFT_REQUIRE(loc32 == 0 || loc32 == 1, "msda_bwd_typed: loc32 %d (0 | 1)", loc32);
    DPFT_REQUIRE(dtype == 0 || workspace, "msda_bwd_typed: 16-bit storage needs the fp32 workspace (N*S*M*D floats)");
    DPFT_REQUIRE(dtype == 0 || ((uintptr_t)workspace & 3) == 0, "msda_bwd_typed: workspace not 4-byte aligned");
    const Dims d{N, S, M, D, Lq, L, P};
    if (dtype == 0)
        return launch_bwd<float, float>(value, shapes, lsi, loc, attn, grad_out, grad_value, grad_loc, grad_attn,
                                        (float*)grad_value, d, stream);
    if (dtype == 1)
        return loc32 ? launch_bwd<_Float16, float>(value, shapes, lsi, loc, attn, grad_out, grad_value, grad_loc, grad_attn, workspace, d, stream)
                     : launch_bwd<_Float16, _Float16>(value, shapes, lsi, loc, attn, grad_out, grad_value, grad_loc, grad_attn, workspace, d, stream);
    return loc32 ? launch_bwd<bf16_t, float>(value, shapes, lsi, loc, attn, grad_out, grad_value, grad_loc, grad_attn, workspace, d, stream)
                 : launch_bwd<bf16_t, bf16_t>(value, shapes, lsi, loc, attn, grad_out, grad_value, grad_loc, grad_attn, workspace, d, stream);
}
