// Fused multi-tensor AdamW (torch.optim.AdamW semantics, decoupled weight decay, no amsgrad) -- one launch
// for all ~1650 parameter tensors instead of the ~10 ms of foreach kernels the reference's
// `getattr(torch.optim, name)` optimizer (src/dprt/training/optimizer.py:6-7) costs per step at 90 M parameters.
#include "common.h"

namespace dpft {

// The 16-byte record the clip-coefficient launch writes and the clipped AdamW launch reads (include/dpft_hip.h).
struct ClipRecord {
    float norm;               // global L2 norm of the active gradients, before clipping
    float coef;               // min(1, max_norm / (norm + 1e-6)); -1 = sit this step out (non-finite norm, "skip" mode)
    int32_t nonfinite;        // this step's sum of squares was not finite
    int32_t nonfinite_total;  // steps skipped for that reason so far ("skip" mode)
};

struct AdamChunk {
    float* p;
    const float* g;
    float* m;
    float* v;
    int32_t n;        // elements in this chunk
    int32_t tensor;   // index into `active`
};

// `skipped[t]` = number of optimizer steps tensor t sat out (no gradient): its own step count is `step - skipped[t]`,
// like the per-parameter `state["step"]` of torch.optim.AdamW.  Only inactive blocks write it (the block of a tensor's
// first chunk), only active blocks read it, so there is no race inside a launch.
// `gate` (round 5, may be null): the step's loss on the device.  The reference steps only `if loss > 0` (training/trainer.py:131);
// the trainer launches backward and optimizer without reading the loss back, and a loss that is not positive closes the gate
// here: every tensor sits the step out exactly as if it had no gradient.
// `CLIP` (dpft_adamw_clip_f32): every gradient element enters the update as g * clip->coef, the coefficient the two norm launches
// below left in the clip record.  The product lives in registers only: the gradient in memory stays unclipped.  coef == 1.0f is
// the unclipped update to the bit (g * 1.0f == g; contracted into an fma the product is exact either way).  A record that asks
// for the step to be skipped (coef < 0: a non-finite norm in "skip" mode) closes the launch exactly as a gate that is not
// positive does.  CLIP = false is the arithmetic of before.
// `EMA` (dpft_adamw_ema_f32): an exponential moving average of the weights, kept in a third flat buffer laid out like the
// moments: the chunk's slice is ema_base + (c.m - m_base), so AdamChunk stays 40 bytes and `ema` has the alignment of `m`.  The
// new p is still in registers when ema += (p - ema) * w is formed (ema.lerp_(p, 1 - d), the rule of
// torch.optim.swa_utils.get_ema_multi_avg_fn): one more read-modify-write per element, no second pass over the weights.
// w = (float)(1 - d_eff), d_eff in double: the configured decay, or with warm-up min(decay, (1 + own) / (10 + own)) with `own`
// the tensor's OWN step count, the one the bias corrections use.  Every block that returns early (closed gate, coef < 0,
// inactive tensor, marker row) returns before it: the average of a tensor advances exactly when the tensor is updated.  p, m
// and v do not depend on it.  EMA = false is the code of before (the four trailing arguments are not read).
template <bool CLIP, bool EMA>
__global__ __launch_bounds__(256) void adamw_kernel(const AdamChunk* __restrict__ chunks, const int32_t* __restrict__ active,
                                                     int32_t* __restrict__ skipped, int32_t step,
                                                     float lr, float beta1, float beta2, float eps, float decay,
                                                     float step_size, float inv_sqrt_bc2, const float* __restrict__ gate,
                                                     const ClipRecord* __restrict__ clip, const float* m_base, float* ema_base,
                                                     float ema_decay, int32_t ema_warmup) {
    const AdamChunk c = chunks[blockIdx.x];
    float coef = 1.f;
    bool closed = gate != nullptr && !(gate[0] > 0.f);
    if (CLIP) {
        coef = clip->coef;
        closed = closed || coef < 0.f;
    }
    if (closed || (active && !active[c.tensor])) {             // parameters without a gradient are skipped (grad is None)
        if (skipped && c.m == nullptr && threadIdx.x == 0) skipped[c.tensor] += 1;   // marker row: one per tensor
        return;
    }
    if (c.m == nullptr) return;                    // marker row of an active tensor
    int32_t own = step;
    if (skipped) {
        own = step - skipped[c.tensor];
        if (own != step) {                         // bias corrections of this tensor's own step count
            const double bc1 = 1.0 - pow((double)beta1, (double)own), bc2 = 1.0 - pow((double)beta2, (double)own);
            step_size = (float)((double)lr / bc1);
            inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
        }
    }
    float* ema = nullptr;
    float w = 0.f;
    if (EMA) {
        ema = ema_base + (c.m - m_base);
        double d_eff = (double)ema_decay;
        if (ema_warmup) d_eff = fmin(d_eff, (1.0 + (double)own) / (10.0 + (double)own));
        w = (float)(1.0 - d_eff);
    }
    for (int i = threadIdx.x * 4; i < c.n; i += 256 * 4) {
        if (i + 3 < c.n && ((((uintptr_t)(c.p + i)) | ((uintptr_t)(c.g + i))) & 15) == 0) {
            f32x4 p = *reinterpret_cast<f32x4*>(c.p + i);
            f32x4 g = *reinterpret_cast<const f32x4*>(c.g + i);
            if (CLIP) g *= coef;
            f32x4 m = *reinterpret_cast<f32x4*>(c.m + i);
            f32x4 v = *reinterpret_cast<f32x4*>(c.v + i);
            f32x4 a;
            if (EMA) a = *reinterpret_cast<f32x4*>(ema + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                p[e] *= decay;
                m[e] = m[e] + (g[e] - m[e]) * (1.f - beta1);           // exp_avg.lerp_(grad, 1 - beta1)
                v[e] = v[e] * beta2 + (1.f - beta2) * g[e] * g[e];
                const float denom = sqrtf(v[e]) * inv_sqrt_bc2 + eps;
                p[e] -= step_size * (m[e] / denom);
                if (EMA) a[e] = a[e] + (p[e] - a[e]) * w;                   // ema.lerp_(p, 1 - d)
            }
            if (EMA) *reinterpret_cast<f32x4*>(ema + i) = a;
            *reinterpret_cast<f32x4*>(c.p + i) = p;
            *reinterpret_cast<f32x4*>(c.m + i) = m;
            *reinterpret_cast<f32x4*>(c.v + i) = v;
        } else {
            for (int e = i; e < min(i + 4, c.n); ++e) {
                float p = c.p[e] * decay;
                const float g = CLIP ? c.g[e] * coef : c.g[e];
                const float m = c.m[e] + (g - c.m[e]) * (1.f - beta1);
                const float v = c.v[e] * beta2 + (1.f - beta2) * g * g;
                p -= step_size * (m / (sqrtf(v) * inv_sqrt_bc2 + eps));
                if (EMA) ema[e] = ema[e] + (p - ema[e]) * w;
                c.p[e] = p; c.m[e] = m; c.v[e] = v;
            }
        }
    }
}

// Sum over a workgroup of 256 threads in a fixed order: the lanes of a wave by halving strides, then the four waves one after
// the other through LDS.  The value is valid in thread 0.
__device__ __forceinline__ double block_sum_256(double acc, double* wave_sums) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = acc;
    __syncthreads();
    return ((wave_sums[0] + wave_sums[1]) + wave_sums[2]) + wave_sums[3];
}

// Gradient clipping by global L2 norm, stage 1: partials[row] = sum of g^2 over the elements of chunk row `row`, one workgroup per
// row of the table adamw_kernel reads, with its `active` flags.  Every element is widened to double BEFORE it is squared: the
// product of two fp32 values is exact in fp64, so 3e19 does not overflow and 1e-30 does not flush, and a kernel that streams 4
// bytes per element is nowhere near the fp64 rate.  16-byte loads where g + i is 16-byte aligned, scalar loads otherwise (the
// split of adamw_kernel).  No atomics: each row has its own slot, a marker row and a row of an inactive tensor write 0.0, so
// the partials -- and everything derived from them -- do not depend on which workgroup finishes when.
__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const AdamChunk* __restrict__ chunks, const int32_t* __restrict__ active,
                                                           double* __restrict__ partials) {
    __shared__ double wave_sums[4];
    const AdamChunk c = chunks[blockIdx.x];
    if (c.m == nullptr || c.n <= 0 || (active && !active[c.tensor])) {      // (uniform over the workgroup)
        if (threadIdx.x == 0) partials[blockIdx.x] = 0.0;
        return;
    }
    double acc = 0.0;
    for (int i = threadIdx.x * 4; i < c.n; i += 256 * 4) {
        if (i + 3 < c.n && (((uintptr_t)(c.g + i)) & 15) == 0) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(c.g + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = (double)g[e];
                acc += d * d;
            }
        } else {
            for (int e = i; e < min(i + 4, c.n); ++e) {
                const double d = (double)c.g[e];
                acc += d * d;
            }
        }
    }
    acc = block_sum_256(acc, wave_sums);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// Stage 2, ONE workgroup: S = sum of partials[0 .. n) -- thread t adds partials[t], partials[t + 256], ... in index order, then
// the fixed tree of block_sum_256: the same bits from run to run -- and the clip record.  norm = (float)sqrt(S); coef is
// torch.nn.utils.clip_grad_norm_'s rule (norm_type 2, error_if_nonfinite=False) evaluated in fp64 and rounded once.  S not
// finite: mode 0 ("propagate") leaves coef to the formula (NaN for a NaN norm, 0 for an infinite one: what torch multiplies the
// gradients by), mode 1 ("skip") writes coef = -1, which closes the clipped AdamW launch, and counts the step.
__global__ __launch_bounds__(256) void grad_clip_coef_kernel(const double* __restrict__ partials, int32_t n, double max_norm,
                                                              int32_t nonfinite_mode, ClipRecord* __restrict__ record) {
    __shared__ double wave_sums[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += partials[i];
    const double S = block_sum_256(acc, wave_sums);
    if (threadIdx.x == 0) {
        const double norm = sqrt(S);
        const bool bad = !isfinite(S);
        const double r = max_norm / (norm + 1e-6);
        float coef = (float)(r >= 1.0 ? 1.0 : r);      // (a NaN compares false and passes through, as through torch's clamp)
        if (bad && nonfinite_mode == 1) {
            coef = -1.f;
            record->nonfinite_total += 1;
        }
        record->norm = (float)norm;
        record->coef = coef;
        record->nonfinite = bad ? 1 : 0;
    }
}

// One row of dpft_swap_f32's table: two disjoint fp32 ranges of n elements that change places.
struct SwapRow {
    float* a;
    float* b;
    int32_t n;
    int32_t pad;
};

// a[0 .. n) <-> b[0 .. n), one workgroup per row: 16-byte accesses where both pointers are 16-byte aligned and four elements
// remain, scalar accesses otherwise (the split of adamw_kernel).  Each element is read and written by one thread only.
__global__ __launch_bounds__(256) void swap_kernel(const SwapRow* __restrict__ rows) {
    const SwapRow r = rows[blockIdx.x];
    for (int i = threadIdx.x * 4; i < r.n; i += 256 * 4) {
        if (i + 3 < r.n && ((((uintptr_t)(r.a + i)) | ((uintptr_t)(r.b + i))) & 15) == 0) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(r.a + i);
            const f32x4 b = *reinterpret_cast<const f32x4*>(r.b + i);
            *reinterpret_cast<f32x4*>(r.a + i) = b;
            *reinterpret_cast<f32x4*>(r.b + i) = a;
        } else {
            for (int e = i; e < min(i + 4, r.n); ++e) {
                const float a = r.a[e], b = r.b[e];
                r.a[e] = b; r.b[e] = a;
            }
        }
    }
}

}  // namespace dpft

using namespace dpft;

extern "C" int dpft_adamw_f32(const void* chunks, int32_t n_chunks, const int32_t* active, int32_t* skipped, float lr,
                              float beta1, float beta2, float eps, float weight_decay, int32_t step, const float* gate,
                              dpft_stream_t stream) {
    DPFT_REQUIRE(chunks && n_chunks > 0 && step >= 1, "adamw: bad arguments");
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    hipLaunchKernelGGL((adamw_kernel<false, false>), dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, (const AdamChunk*)chunks, active, skipped,
                       step, lr, beta1, beta2, eps, (float)(1.0 - (double)lr * weight_decay), (float)(lr / bc1),
                       (float)(1.0 / sqrt(bc2)), gate, (const ClipRecord*)nullptr, (const float*)nullptr, (float*)nullptr, 0.f, 0);
    return check_launch("adamw");
}

extern "C" int dpft_adamw_clip_f32(const void* chunks, int32_t n_chunks, const int32_t* active, int32_t* skipped, float lr,
                                   float beta1, float beta2, float eps, float weight_decay, int32_t step, const float* gate,
                                   const void* record, dpft_stream_t stream) {
    DPFT_REQUIRE(chunks && n_chunks > 0 && step >= 1 && record, "adamw_clip: bad arguments");
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    hipLaunchKernelGGL((adamw_kernel<true, false>), dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, (const AdamChunk*)chunks, active, skipped,
                       step, lr, beta1, beta2, eps, (float)(1.0 - (double)lr * weight_decay), (float)(lr / bc1),
                       (float)(1.0 / sqrt(bc2)), gate, (const ClipRecord*)record, (const float*)nullptr, (float*)nullptr, 0.f, 0);
    return check_launch("adamw_clip");
}

extern "C" int dpft_adamw_ema_f32(const void* chunks, int32_t n_chunks, const int32_t* active, int32_t* skipped, float lr,
                                  float beta1, float beta2, float eps, float weight_decay, int32_t step, const float* gate,
                                  const void* record, const float* m_base, float* ema_base, float ema_decay, int32_t ema_warmup,
                                  dpft_stream_t stream) {
    DPFT_REQUIRE(chunks && n_chunks > 0 && step >= 1 && m_base && ema_base, "adamw_ema: bad arguments");
    DPFT_REQUIRE(ema_decay >= 0.f && ema_decay < 1.f, "adamw_ema: ema_decay %g is not in [0, 1)", (double)ema_decay);
    DPFT_REQUIRE(ema_warmup == 0 || ema_warmup == 1, "adamw_ema: ema_warmup %d (0 off | 1 on)", ema_warmup);
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    const float decay = (float)(1.0 - (double)lr * weight_decay), step_size = (float)(lr / bc1), inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    if (record)
        hipLaunchKernelGGL((adamw_kernel<true, true>), dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, (const AdamChunk*)chunks,
                           active, skipped, step, lr, beta1, beta2, eps, decay, step_size, inv_sqrt_bc2, gate,
                           (const ClipRecord*)record, m_base, ema_base, ema_decay, ema_warmup);
    else
        hipLaunchKernelGGL((adamw_kernel<false, true>), dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, (const AdamChunk*)chunks,
                           active, skipped, step, lr, beta1, beta2, eps, decay, step_size, inv_sqrt_bc2, gate,
                           (const ClipRecord*)nullptr, m_base, ema_base, ema_decay, ema_warmup);
    return check_launch("adamw_ema");
}

extern "C" int dpft_swap_f32(const void* rows, int32_t n_rows, dpft_stream_t stream) {
    DPFT_REQUIRE(rows && n_rows > 0, "swap: bad arguments");
    hipLaunchKernelGGL(swap_kernel, dim3(n_rows), dim3(256), 0, (hipStream_t)stream, (const SwapRow*)rows);
    return check_launch("swap");
}

extern "C" int dpft_grad_sqnorm_f32(const void* chunks, int32_t n_chunks, const int32_t* active, double* partials,
                                    dpft_stream_t stream) {
    DPFT_REQUIRE(chunks && n_chunks > 0 && partials, "grad_sqnorm: bad arguments");
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, (const AdamChunk*)chunks, active, partials);
    return check_launch("grad_sqnorm");
}

extern "C" int dpft_grad_clip_coef_f32(const double* partials, int32_t n_partials, float max_norm, int32_t nonfinite_mode,
                                       void* record, dpft_stream_t stream) {
    DPFT_REQUIRE(partials && n_partials > 0 && record, "grad_clip_coef: bad arguments");
    DPFT_REQUIRE(max_norm > 0.f && max_norm <= 3.402823466e38f, "grad_clip_coef: max_norm %g is not finite and positive", (double)max_norm);
    DPFT_REQUIRE(nonfinite_mode == 0 || nonfinite_mode == 1, "grad_clip_coef: nonfinite_mode %d (0 propagate | 1 skip)", nonfinite_mode);
    hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, n_partials, (double)max_norm,
                       nonfinite_mode, (ClipRecord*)record);
    return check_launch("grad_clip_coef");
}
