/* dpft_hip.h -- C-ABI of libdpft_hip.so (gfx950 / MI355X).
 *
 * This is the drop-in boundary for the DPFT hot path.  Every entry point is a
 * plain C function over raw device pointers + sizes + a hipStream_t; no torch types.  Rules:
 *   - the caller owns every buffer (inputs, outputs, workspaces); nothing is allocated inside;
 *   - no hidden synchronisation: every call only enqueues work on `stream` (graph-capturable);
 *   - re-entrant and stream-ordered;
 *   - return 0 on success, a negative code otherwise; dpft_last_error() returns the message of
 *     the last failure on the calling thread (the Python side raises RuntimeError from it).
 *   - sampling locations (dpft_msda_*, dpft_xattn_*, dpft_xattn_ffn_train_*, dpft_decoder_forward_f32) must be finite
 *     and below 2^31 pixels in magnitude on every level: the fused decoders convert floor(t) to int before they
 *     apply the in-map mask (sampling rule; tested out to 2^20 pixels on both sides).
 *
 * Reference interfaces replaced (paths relative to the TUMFTM/DPFT checkout):
 *   dpft_msda_fwd_f32 / dpft_msda_bwd_f32
 *       MSDA.ms_deform_attn_forward / ms_deform_attn_backward, the only native seam the
 *       reference has: src/dprt/models/layers/ms_deform_attn.py:24,32-39,58-66.
 *   dpft_msda_fwd_typed / dpft_msda_bwd_typed
 *       the same seam with fp32, half or bf16 storage (upstream's extension takes half too: the door mixed-precision
 *       training comes through).
 *   dpft_xattn_fwd_f32 / dpft_xattn_bwd_f32
 *       the flatten+cat -> value_proj -> MSDA core chain of MLFusion.forward_cross_attn /
 *       MSDeformAttn.forward: src/dprt/models/fusers/mpfusion.py:150-208 and
 *       src/dprt/models/layers/ms_deform_attn.py:172-213 ("sample-then-project", reads the
 *       NHWC FPN levels in place).
 *   dpft_conv2d_nhwc_{fwd,dgrad,wgrad}_f32, dpft_bn_*, dpft_maxpool_*, dpft_bn_add_relu_*
 *       the cuDNN kernels torch dispatches for the torchvision ResNet body and FPN:
 *       src/dprt/models/backbones/resnet.py:47-55,80-107, src/dprt/models/necks/fpn.py:39-43,70-83.
 *   dpft_fpn_topdown_*, dpft_add_pos_*
 *       F.interpolate(nearest)+add inside torchvision FPN, and the in-place sinusoidal
 *       embedding src/dprt/models/embeddings/sinusoidal.py:63-110.
 *   dpft_giou3d_yaw_f32
 *       pytorch3d.ops.box3d_overlap as used by src/dprt/utils/iou.py:121-210.
 */
#ifndef DPFT_HIP_H
#define DPFT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPFT_OK 0
#define DPFT_ERR_ARG (-1)
#define DPFT_ERR_LAUNCH (-2)
#define DPFT_ERR_UNSUPPORTED (-3)

typedef void* dpft_stream_t; /* hipStream_t */

int dpft_version(void);
const char* dpft_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Convolution family: NHWC activations, weights physically [Cout][kh][kw][Cin]
 * (= torch OIHW tensor in channels_last memory format), fp32, MFMA implicit GEMM.
 * ---------------------------------------------------------------------------------------- */
typedef struct dpft_conv_desc {
    int32_t B, H, W, C;      /* input  (B,H,W,C)                      */
    int32_t K;               /* output channels                       */
    int32_t kh, kw, stride, pad;
    int32_t OH, OW;          /* output spatial size                   */
    int32_t act16;           /* 0: activations (x, y, dy, dx, residual sources) are fp32 tensors;
                              * 1: they are bf16 tensors ("bf16 mixed precision" storage of BASELINE.json configs[4]:
                              *    4 channels = 8 bytes per loader lane, BatchNorm statistics still from the fp32
                              *    accumulators); weights, weight gradients, BN blocks and statistics stay fp32.
                              *    Needs C % 64 == 0 and K % 64 == 0; the pointers are still declared const float*.  */
    /* Round 5: the GEMM operands as THREE bf16 PLANES (dpft_split_planes_f32: an fp32 value is exactly the sum of three bf16
     * terms; plane p of element e at base + 2 (p E + e) bytes, E = the tensor's element count).  When BOTH are given and the
     * problem takes the C % 64 == 0 path without an operand prologue, the forward / data-gradient GEMM reads its operands
     * from them and multiplies on the bf16 matrix cores (six term products, fp32 accumulation: fp32-grade results at a
     * multiple of the fp32 MFMA rate, dpft_amd/csrc/conv_x3.hip).  a_planes = planes of the A operand (x of the forward,
     * dy of the data gradient), w_planes = planes of the weight tensor passed as w / w_t.  The fp32 tensors are still
     * required (fallback paths, epilogues).  NULL = fp32 operands (zero-initialise the descriptor). */
    const void* a_planes;
    const void* w_planes;
} dpft_conv_desc;

/* bytes of workspace dpft_conv2d_* may need for this problem: a ticket header + split-K partial slabs.
 * Contract (round 4): the first dpft_conv2d_workspace_header_bytes() bytes of a workspace buffer must be ZERO when the
 * buffer is first handed to the library (dpft_conv2d_workspace_init zero-fills them on `stream`); every call leaves
 * them zero again, so one initialisation per buffer is enough.  The header holds one ticket per output tile of a
 * split-K launch: the workgroup that draws a tile's last ticket sums the partial tiles in split order and runs the
 * whole epilogue -- there is no separate reduction launch.  Calls that share a workspace must be stream-ordered. */
int64_t dpft_conv2d_workspace_bytes(const dpft_conv_desc* d);
int64_t dpft_conv2d_workspace_header_bytes(void);
int dpft_conv2d_workspace_init(void* workspace, dpft_stream_t stream);
/* fp32 tensor of n elements (n % 4 == 0) -> three bf16 planes [3][n]: plane 0 = RNE bf16 of the value, plane 1 = RNE bf16 of
 * what plane 0 left, plane 2 = the (exact) rest.  src = plane0 + plane1 + plane2 exactly. */
int dpft_split_planes_f32(const float* src, void* planes, int64_t n, dpft_stream_t stream);
/* number of M-tiles the forward kernel uses for its fused BN-statistics epilogue
 * (rows of the `stats` buffer: stats is [mtiles][2][K] floats = per-tile mean and M2);
 * *tile_rows receives the tile height so the caller can recover per-tile counts. */
int32_t dpft_conv2d_stats_tiles(const dpft_conv_desc* d, int32_t* tile_rows);

/* The kernel family (numbering of dpft_profile_get_family) the launch plan names for this problem in the current compute mode:
 * kind 0 forward, 1 data gradient, 2 weight gradient; has_workspace as the launch would be given one.  For a strided data
 * gradient run as parity classes: the family of the last class that launches (what its profile record holds).  Decided on the
 * host from the descriptor alone -- nothing is launched; -1 on a bad descriptor or kind. */
int32_t dpft_conv2d_planned_family(const dpft_conv_desc* d, int32_t kind, int32_t has_workspace);

/* Arithmetic of the forward / data-gradient GEMMs of every conv with C % 64 == 0 and of the 128 x 128-tiled weight
 * gradients (process-wide; call between launches):
 *   0  fp32 operands, fp32 accumulation -- the reference's arithmetic (config/kradar.json "dtype": "float32"), default;
 *   1  operands rounded to bf16 (RNE) on their way into LDS, fp32 accumulation (v_mfma_f32_32x32x16_bf16); tensors in
 *      memory, BatchNorm, the small weight gradients, optimizer stay fp32 ("bf16 mixed precision", BASELINE.json configs[4]).
 *   2  (experimental, forward / data gradient only) every operand value split into three bf16 terms on its way into
 *      LDS and the six term products of weight >= 2^-16 accumulated in fp32 on the bf16 matrix cores: fp32-grade
 *      results (measured 2-3e-7 relative L2 error vs fp64, the fp32 MFMA path 6-8e-7), 10-15 % faster than mode 0.
 * Returns DPFT_ERR_ARG for any other value. */
int dpft_conv_set_compute(int32_t mode);
int32_t dpft_conv_get_compute(void);
/* fp32 compute mode only: run the big multi-tap GEMMs (3x3 / 7x7 filters, C % 64 == 0, >= 2 GFLOP) as 3 x bf16 split products
 * on the bf16 matrix cores -- fp32 tensors in, fp32 results out, six exact term products per fp32 product accumulated in
 * fp32 (dpft_amd/csrc/conv_x3.hip; error vs fp64 below the fp32 MFMA path's).  Default on (DPFT_CONV_SPLIT=0 presets off);
 * off = v_mfma_f32_32x32x2_f32 everywhere.  Set before problems are sized: dpft_conv2d_stats_tiles depends on it. */
int dpft_conv_set_split(int32_t on);
int32_t dpft_conv_get_split(void);

/* BN parameter block convention used across the library: bnp[4][K] floats =
 *   row 0 mean, row 1 scale = gamma*invstd, row 2 beta, row 3 invstd;   bn(v) = (v - mean)*scale + beta
 * (mean is subtracted first: no beta - mean*scale cancellation when |mean| >> std). */

/* y[B,OH,OW,K] = conv(act(x), w) (+bias).  Optional fused prologue on the input operand:
 * act(x) = [max(., 0)] bn(x) with the PRODUCER's BN block pro_bn[4][C] (NULL = identity; pro_relu
 * selects the max).  Padding stays exactly zero.  Optional fused epilogue: per-M-tile per-channel
 * (mean, M2) of y into `stats` for train-mode BatchNorm (NULL to skip).  DPFT_ERR_ARG for bf16 weights (act16 = 2) with a bias
 * or a prologue, and for statistics of a problem the streaming 1x1 kernel takes (the tiling dpft_conv2d_stats_tiles reports)
 * together with a bias or a prologue without the ReLU. */
int dpft_conv2d_nhwc_fwd_f32(const dpft_conv_desc* d, const float* x, const float* w,
                             const float* bias, const float* pro_bn, int32_t pro_relu, float* y,
                             float* stats, void* workspace, dpft_stream_t stream);
/* Inference form of conv + BatchNorm (+ residual add) (+ ReLU) -- what torchvision's Bottleneck.forward computes in eval
 * mode per conv (resnet.py Bottleneck: conv -> bn -> relu, and conv3 -> bn3 -> += identity -> relu; reached through
 * src/dprt/models/backbones/resnet.py:80-107):  y = [relu](bn(conv(x, w)) [+ residual]),  out_bn = BN block [4][K] of the
 * output channels (dpft_bn_eval_params_f32).  One launch where the problem takes the C % 64 == 0 path without split-K
 * (applied in the GEMM epilogue), otherwise the convolution followed by dpft_bn_act_f32 in place: same arithmetic.
 * K % 4 == 0 (both forms take the output channels four at a time): DPFT_ERR_ARG otherwise, before anything is launched. */
int dpft_conv2d_nhwc_fwd_bnact_f32(const dpft_conv_desc* desc, const float* x, const float* w, const float* out_bn,
                                   int32_t relu, const float* residual, float* y, void* workspace, dpft_stream_t stream);

/* dx[B,H,W,C] (+)= conv_transpose(dy, w).  w_t is the transposed weight [C][kh][kw][K]
 * (see dpft_weight_transpose_f32); accumulate != 0 adds into dx instead of overwriting it. */
int dpft_conv2d_nhwc_dgrad_f32(const dpft_conv_desc* d, const float* dy, const float* w_t,
                               float* dx, int32_t accumulate, void* workspace,
                               dpft_stream_t stream);

/* Data gradient with the FIRST PASS of a BatchNorm backward in its epilogue -- the form the ResNet launch plan
 * (dpft_resnet_backward_stage) runs: the tensor this call writes, dx (B,H,W,C), is the `dout` of a BatchNorm layer
 * whose input bn_y has the same shape and whose BN block (mean, gamma*invstd, beta, invstd) is bn_block [4][C];
 * with d = dx under that layer's ReLU mask (bn_mask8: one byte per 4 channels, bit e = element e passed; or
 * bn_self_mask: mask = bn(bn_y) > 0) the launch adds  sums[0][c] += sum_pixels d,  sums[1][c] += sum_pixels d * xhat,
 * xhat = (bn_y - mean) * invstd  -- what dpft_bn_bwd_reduce_f32 computes in a pass of its own.  sums [2][C] must be
 * zero (or hold a running total).  *applied = 1 when the launch carried the reduction; 0 when the problem takes a path
 * that cannot (split-K, thin channels, a strided 1x1 whose parity classes leave pixels untouched): sums is then
 * untouched and the caller runs the separate pass.
 * res_src != NULL: the bottleneck's identity branch folded in as well, dx = dgrad(dy) + (mask ? res_src : 0) with the
 * mask from res_mask8 (bytes) or res_out > 0 (the block output; always required for the split-K form); stride 1 only. */
int dpft_conv2d_nhwc_dgrad_bn_reduce_f32(const dpft_conv_desc* d, const float* dy, const float* w_t, float* dx,
                                         int32_t accumulate, const float* res_src, const float* res_out,
                                         const uint8_t* res_mask8, const float* bn_y, const float* bn_block,
                                         const uint8_t* bn_mask8, int32_t bn_self_mask, float* sums,
                                         int32_t* applied, void* workspace, dpft_stream_t stream);
/* dw[K][kh][kw][C] = sum_pixels dy (x) act(x); same optional prologue on x as forward.
 * dw is overwritten.  The prologue rides on the vector kernels only: C % 32 == 0 and K % 4 == 0, DPFT_ERR_ARG otherwise. */
int dpft_conv2d_nhwc_wgrad_f32(const dpft_conv_desc* d, const float* x, const float* dy,
                               const float* pro_bn, int32_t pro_relu, float* dw, void* workspace,
                               dpft_stream_t stream);
/* [K][taps][C] -> [C][taps][K] */
int dpft_weight_transpose_f32(const float* w, float* w_t, int32_t K, int32_t taps, int32_t C,
                              dpft_stream_t stream);
/* The same for n (<= 80) weight tensors in ONE launch: w[i] is [K[i]][taps[i]][C[i]], w_t[i] receives [C[i]][taps[i]][K[i]]
 * (an FPN's ten convs per backward, `necks/fpn.py:39-43`; pointer / size arrays live on the host). */
int dpft_weight_transpose_batch_f32(int32_t n, const float* const* w, float* const* w_t, const int32_t* K,
                                    const int32_t* taps, const int32_t* C, dpft_stream_t stream);
/* dw as dpft_conv2d_nhwc_wgrad_f32 (no prologue) AND db = the bias gradient of a conv with bias (`necks/fpn.py:39-43`:
 * torchvision's FPN convs), in one pass over dy where the weight-gradient kernel has dy at hand. */
int dpft_conv2d_nhwc_wgrad_bias_f32(const dpft_conv_desc* d, const float* x, const float* dy, float* dw, float* db,
                                    void* workspace, dpft_stream_t stream);
/* db[K] = sum over rows of dy[M][K] */
int dpft_bias_grad_f32(const float* dy, float* db, int64_t M, int32_t K, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * BatchNorm (train + eval), ReLU, residual, max-pool on NHWC fp32
 * ---------------------------------------------------------------------------------------- */
/* standalone per-tile statistics of y[M][K] in the same [tiles][2][K] format (tile_rows rows each) */
int dpft_bn_stats_f32(const float* y, float* stats, int64_t M, int32_t K, int32_t tile_rows,
                      dpft_stream_t stream);
/* combine tiles (Chan's parallel variance), write the BN block bnp[4][K], update the running
 * statistics (momentum; unbiased variance) when running_mean != NULL. */
int dpft_bn_finalize_f32(const float* stats, int32_t tiles, int32_t tile_rows, int64_t M, int32_t K,
                         const float* gamma, const float* beta, float eps, float momentum,
                         float* running_mean, float* running_var, float* bnp, dpft_stream_t stream);
/* eval mode: BN block from the running statistics */
int dpft_bn_eval_params_f32(const float* gamma, const float* beta, const float* running_mean,
                            const float* running_var, float eps, int32_t K, float* bnp,
                            dpft_stream_t stream);
/* out = [relu]( bn(y)  [+ (bn_res(res) | res)] ) elementwise over [M][K] */
int dpft_bn_act_f32(const float* y, const float* bnp, const float* res, const float* res_bnp,
                    int32_t relu, float* out, int64_t M, int32_t K, dpft_stream_t stream);
/* stem: out[B,PH,PW,K] = maxpool3x3s2p1( relu(bn(y)) ), y is [B,H,W,K] */
int dpft_bn_relu_maxpool_f32(const float* y, const float* bnp, float* out, int32_t B, int32_t H,
                             int32_t W, int32_t K, int32_t PH, int32_t PW, dpft_stream_t stream);
/* backward of the stem pool + ReLU: dz[B,H,W,K] = grad wrt bn(y) = (relu(bn(y))>0) * sum of dout over
 * the pool windows whose first arg-max (scan order, strict >) is this pixel */
int dpft_bn_relu_maxpool_bwd_f32(const float* y, const float* bnp, const float* dout, float* dz,
                                 int32_t B, int32_t H, int32_t W, int32_t K, int32_t PH, int32_t PW,
                                 dpft_stream_t stream);
/* BatchNorm backward, two passes.  dz = dout * mask with
 *   mask = (out > 0)              if out != NULL       (out = post-activation tensor)
 *   mask = (bn_mask(y) > 0)       elif mask_bnp != NULL (recompute the fused ReLU from its BN block)
 *   mask = 1                      otherwise.
 * pass 1: sums[0][k] = sum dz, sums[1][k] = sum dz * xhat   (xhat = (y-mean)*invstd from bnp) */
int dpft_bn_bwd_reduce_f32(const float* y, const float* dout, const float* out,
                           const float* mask_bnp, const float* bnp, float* sums, int64_t M,
                           int32_t K, dpft_stream_t stream);
/* pass 2: dy = gamma*invstd*(dz - sums0/M - xhat*sums1/M); dgamma = sums1, dbeta = sums0 */
int dpft_bn_bwd_apply_f32(const float* y, const float* dout, const float* out,
                          const float* mask_bnp, const float* bnp, const float* gamma,
                          const float* sums, float* dy, float* dgamma, float* dbeta, int64_t M,
                          int32_t K, dpft_stream_t stream);
/* dz = dout * (out > 0)  (residual branch gradient) */
int dpft_relu_bwd_f32(const float* dout, const float* out, float* dz, int64_t n,
                      dpft_stream_t stream);
/* a += b */
int dpft_add_inplace_f32(float* a, const float* b, int64_t n, dpft_stream_t stream);

/* The same passes with everything the launch plan passes its workers, so that every kernel form can be driven alone (the
 * entries above are these with storage = 0 and no optional tensor).
 *   storage   0: the activation / gradient tensors (y, res, out, dout, dy) are fp32; 1: bf16 (mixed-precision storage).  BN
 *             blocks, sums, parameter gradients, out32 and masks keep their types; all arithmetic is fp32 either way.
 *   mask8     [M][K/4] bytes, bit e of a byte = element e of its 4 channels is > 0 in `out`: written by the forward pass, read
 *             by the backward passes INSTEAD of `out` (precedence: mask8, then out, then mask_bnp).
 *   out32     optional fp32 copy of `out` (bf16 storage: the unrounded values).
 * Refused with DPFT_ERR_ARG: K % 4 != 0, null tensors, res_bnp without res, a storage other than 0 / 1, tensors that are not
 * aligned to 4 elements. */
int dpft_bn_act_any_f32(const void* y, const float* bnp, const void* res, const float* res_bnp, int32_t relu, void* out,
                        float* out32, uint8_t* mask8, int64_t M, int32_t K, int32_t storage, dpft_stream_t stream);
/* fp32 tensors; either BatchNorm given as column sums instead of a BN block: y_sums / res_sums are [4][K] 64-bit words, the
 * 96-bit fixed-point accumulators the forward convs add to (sum y: high word counting fours, low word in units of 2^-46; then
 * sum y^2 the same way) over the M rows, with the layer's gamma / beta; eps shared by both.  A null sums pointer = take that
 * side's BN block.  *used = 0 and NOTHING launched (out untouched) where only the generic kernel fits the shape: the caller
 * finalizes the sums into BN blocks and calls dpft_bn_act_f32. */
int dpft_bn_act_sums_f32(const float* y, const float* bnp, const uint64_t* y_sums, const float* y_gamma, const float* y_beta,
                         const float* res, const float* res_bnp, const uint64_t* res_sums, const float* res_gamma,
                         const float* res_beta, float eps, int32_t relu, float* out, uint8_t* mask8, int64_t M,
                         int32_t K, int32_t* used, dpft_stream_t stream);
/* dpft_conv2d_nhwc_fwd_f32 with the train-mode statistics as column sums (the accumulators described above), one launch:
 *   sums           [4][K] words (may be NULL; needs `stats` and `sums_used`), zero before the first launch that adds to them.
 *                  *sums_used = 1: the launch added n * mean and M2 + n * mean^2 of every statistics tile to them INSTEAD of
 *                  writing `stats`; 0: they are untouched and `stats` holds the per-tile table (a bias, the generic kernel, a
 *                  K split finished by a reduction launch, K % 4 != 0).
 *   pro_sums       (may be NULL) the prologue's BatchNorm as column sums [4][C] of the producer over its pro_rows rows, with
 *                  its gamma / beta / eps; `pro_bn` must still be given.  DPFT_ERR_ARG where the kernel of this conv builds no
 *                  prologue from sums; *pro_sums_used = 1 where it did. */
int dpft_conv2d_nhwc_fwd_sums_f32(const dpft_conv_desc* d, const float* x, const float* w, const float* bias,
                                  const float* pro_bn, int32_t pro_relu, float* y, float* stats, uint64_t* sums,
                                  int32_t* sums_used, const uint64_t* pro_sums, const float* pro_gamma, const float* pro_beta,
                                  int64_t pro_rows, float pro_eps, int32_t* pro_sums_used, void* workspace, dpft_stream_t stream);
/* column sums -> BN block bnp[i][4][K[i]] and running statistics (momentum; unbiased variance; running_mean / running_var or
 * their entries may be NULL) of n layers in one launch, sums[i] over M[i] rows.  1 <= n <= 48: DPFT_ERR_ARG otherwise. */
int dpft_bn_finalize_sums_f32(int32_t n, const uint64_t* const* sums, const float* const* gamma, const float* const* beta,
                              float* const* running_mean, float* const* running_var, float* const* bnp, const int64_t* M,
                              const int32_t* K, float eps, float momentum, dpft_stream_t stream);
/* pass 1 (sums [2][K] cleared by the entry) */
int dpft_bn_bwd_reduce_any_f32(const void* y, const void* dout, const void* out, const float* mask_bnp, const uint8_t* mask8,
                               const float* bnp, float* sums, int64_t M, int32_t K, int32_t storage, dpft_stream_t stream);
/* pass 2.  frozen != 0: running-statistics BatchNorm, dy = gamma * invstd * dz (no mean terms); dgamma / dbeta (either may be
 * null) are copied from the sums in both modes.  zero_buf[0..zero_n) is cleared by the same launch (the launch plan's other
 * accumulator); it must not be `sums`. */
int dpft_bn_bwd_apply_any_f32(const void* y, const void* dout, const void* out, const float* mask_bnp, const uint8_t* mask8,
                              const float* bnp, const float* gamma, const float* sums, void* dy, float* dgamma, float* dbeta,
                              float* zero_buf, int32_t zero_n, int64_t M, int32_t K, int32_t storage, int32_t frozen,
                              dpft_stream_t stream);
/* stem pool: y and dz fp32; storage is the type of the pooled tensors `out` / `dout` */
int dpft_bn_relu_maxpool_any_f32(const float* y, const float* bnp, void* out, int32_t B, int32_t H, int32_t W, int32_t K,
                                 int32_t PH, int32_t PW, int32_t storage, dpft_stream_t stream);
int dpft_bn_relu_maxpool_bwd_any_f32(const float* y, const float* bnp, const void* dout, float* dz, int32_t B, int32_t H,
                                     int32_t W, int32_t K, int32_t PH, int32_t PW, int32_t storage, dpft_stream_t stream);
/* a (storage type) += b (fp32); bf16: n % 4 == 0, one rounding to nearest even of the fp32 sum */
int dpft_add_inplace_any_f32(void* a, const float* b, int64_t n, int32_t storage, dpft_stream_t stream);
/* dst (bf16) = src (fp32), round to nearest even; n % 4 == 0 */
int dpft_cvt_f32_bf16(const float* src, void* dst, int64_t n, dpft_stream_t stream);
/* The kernel form the dispatch took at the last launch of this family in the process, written by the dispatch code at the
 * launch (not derived from the shape; as dpft_profile_get_family).  Not thread-safe: a test aid. */
#define DPFT_BN_FORM_NONE 0
#define DPFT_BN_FORM_GENERIC 1          /* channel index per element: every fp32 / 8-byte bf16 kernel, gather pool, reduce */
#define DPFT_BN_FORM_FIXC1 2            /* fp32 fixed-channel, 1 quad per thread and trip */
#define DPFT_BN_FORM_FIXC2 3
#define DPFT_BN_FORM_FIXC3 4
#define DPFT_BN_FORM_WIDE16 5           /* bf16 with 16-byte accesses */
#define DPFT_BN_FORM_WIDE16_FIXC 6
#define DPFT_BN_FORM_POOL_TILED 7       /* tiled max-pool backward */
#define DPFT_BN_FORM_SUMS_TAKEN 8       /* dpft_bn_act_sums_f32 launched its kernel */
#define DPFT_BN_FORM_SUMS_DECLINED 9    /* ... or left the pass to the caller */
int dpft_bn_last_form(int32_t* form);
/* The launch a pass would make, without making it (host only, no device needed; as dpft_conv2d_planned_family): the plan the
 * entries above build and launch from.  `pass`: DPFT_BN_PASS_*.  M rows of K channels; the pool backward takes the batch in M
 * and its input map in H, W (the other passes ignore H, W).  `flags`: DPFT_BN_PLAN_OUT32 an fp32 copy is asked for (act),
 * DPFT_BN_PLAN_ALIGNED16 what the entries test on their pointers: every tensor 16-byte aligned, the mask bytes 2-byte (act,
 * apply; bf16).  `switches`: the five dispatch switches to plan under; NULL = the process's own (its DPFT_* environment). */
#define DPFT_BN_PASS_ACT 0
#define DPFT_BN_PASS_ACT_SUMS 1         /* dpft_bn_act_sums_f32 (fp32 only) */
#define DPFT_BN_PASS_REDUCE 2
#define DPFT_BN_PASS_APPLY 3
#define DPFT_BN_PASS_POOL_BWD 4
#define DPFT_BN_PLAN_OUT32 1
#define DPFT_BN_PLAN_ALIGNED16 2
typedef struct dpft_bn_switches {       /* DPFT_BN_FIXC, DPFT_BN_WIDE16, DPFT_BN_FAT, DPFT_POOL_BWD_TILED, DPFT_EW_BLOCKS_PER_CU */
    int32_t fixc, wide16, fat, pool_bwd_tiled, ew_blocks_per_cu;
} dpft_bn_switches;
typedef struct dpft_bn_plan {
    int32_t form;                       /* DPFT_BN_FORM_* */
    int32_t per_thread;                 /* quads (16-byte bf16 forms: octets; reduce: rows) per thread and trip */
    int64_t grid_x;                     /* workgroups of 256 threads; 0: nothing is launched (column sums declined) */
    int32_t grid_y;
    int32_t lds_bytes;                  /* dynamic LDS */
    int32_t slab, slabs, groups;        /* reduce: channel quads per slab, slabs (= grid_y), row groups per workgroup */
    int64_t rows_per_block;             /* reduce */
} dpft_bn_plan;
int dpft_bn_plan_query(int32_t pass, int64_t M, int32_t K, int32_t H, int32_t W, int32_t storage, int32_t flags,
                       const dpft_bn_switches* switches, dpft_bn_plan* plan);

/* ------------------------------------------------------------------------------------------
 * Native launch plan of the ResNet body (conv1/bn1/relu/maxpool/layer1..n of torchvision's
 * ResNet-50/101/152 behind IntermediateLayerGetter, src/dprt/models/backbones/resnet.py:54-55,
 * incl. the optional 1x1 adjustment conv :47-52).  One call enqueues a whole forward, or the
 * backward of one stage; everything lives in a caller-owned arena; nothing is allocated or
 * synchronised inside (hipGraph-capturable).
 * ---------------------------------------------------------------------------------------- */
typedef struct dpft_resnet_desc {
    int32_t B, H, W, in_channels;   /* NHWC input (B,H,W,in_channels); != 3 adds the adjustment conv */
    int32_t depths[4];              /* bottlenecks per stage, e.g. {3,4,23,3}                       */
    int32_t n_layers;               /* stages to run (multi_scale), 1..4                            */
    float eps, momentum;            /* BatchNorm2d hyper-parameters (1e-5, 0.1)                     */
    int32_t act16;                  /* 1: bf16 activation / gradient storage inside the body (dpft_conv_desc.act16;
                                     * with dpft_conv_set_compute(1) = the mixed precision of BASELINE.json configs[4]);
                                     * input image, stem conv output, stage outputs handed to the caller, all
                                     * parameters, BatchNorm statistics and parameter gradients stay fp32          */
} dpft_resnet_desc;

/* Pointer tables in plan order.  conv: [adjustment], stem conv1, then per bottleneck conv1, conv2,
 * conv3, [downsample.0].  bn: stem bn1, then per bottleneck bn1, bn2, bn3, [downsample.1].
 * Weights are physical [K][kh][kw][C]; *_dw / bn_d* are written (overwritten) by the backward. */
typedef struct dpft_resnet_tables {
    void* const* conv_w;
    void* const* conv_dw;
    void* const* bn_gamma;
    void* const* bn_beta;
    void* const* bn_rm;
    void* const* bn_rv;
    void* const* bn_dgamma;
    void* const* bn_dbeta;
} dpft_resnet_tables;

int64_t dpft_resnet_plan_create(const dpft_resnet_desc* desc);   /* 0 on error */
void dpft_resnet_plan_destroy(int64_t plan);
/* what: 0 arena bytes, 1 #convs, 2 #bns, 3 float offset of stage output idx in the arena,
 *       4 shape entry (idx = stage*4 + dim of (B,H,W,C)), 5 floats kept for backward */
int64_t dpft_resnet_plan_query(int64_t plan, int32_t what, int32_t idx);
/* x (B,H,W,in_channels).  train = 1: batch statistics + running-stat update, activations kept for the backward stages;
 * train = 2: frozen BatchNorm -- activations kept as well, but every BatchNorm normalises with its running statistics
 * (nothing is updated) and the backward stages drop the batch-statistics terms (dy = gamma invstd d): the gradient through
 * an eval-mode body / torchvision's FrozenBatchNorm2d; train = 0: inference (BatchNorm folded into the conv epilogues). */
int dpft_resnet_forward(int64_t plan, const float* x, const dpft_resnet_tables* tables, void* arena,
                        int32_t train, dpft_stream_t stream);
/* Backward of stage `stage` (call n_layers-1 ... 0 after a train forward; stage 0 also runs the
 * stem).  dout = external gradient of that stage's output (NULL = none).  frozen = the BatchNorm mode of the forward this
 * backward belongs to (1: it ran with train = 2, running statistics; 0: train = 1) -- the caller says it, the plan keeps
 * no per-forward state. */
int dpft_resnet_backward_stage(int64_t plan, int32_t stage, const float* x,
                               const dpft_resnet_tables* tables, void* arena, const float* dout,
                               int32_t frozen, dpft_stream_t stream);
/* The stream the plan's weight-gradient GEMMs run on while the data-gradient chain continues on the caller's stream
 * (default: a stream the plan creates on first use).  Passing the caller's own stream keeps everything in order on it. */
int dpft_resnet_plan_set_side_stream(int64_t plan, dpft_stream_t side);
/* on != 0: a train-mode forward and each backward stage are captured into hipGraphs (after two eager calls per argument
 * set) and replayed -- one host-side launch instead of several hundred.  Only calls that are a single-stream sequence are
 * captured (the forward always; a backward stage when the weight-gradient stream IS the launch stream); the caller must
 * keep x / arena / dout / the tables' pointers the same from call to call (a new set is captured anew). */
int dpft_resnet_plan_set_graph(int64_t plan, int32_t on);

/* ------------------------------------------------------------------------------------------
 * Streams on distinct hardware queues (MI355X-side addition; the reference is single-stream).
 * The runtime multiplexes HIP streams onto 4 hardware queues and streams sharing a queue run in order; the step's
 * concurrency (camera chain | its weight gradients | radar encoders) needs one queue each.  out[0..n-1] receive streams
 * (library-owned, never destroyed) that share a queue neither with main_stream nor with each other -- found by probing
 * with a spin kernel; when the device has fewer queues the entries repeat.  Returns the number of distinct queues found
 * or a negative error code.  Synchronises the device: set-up time only.
 * ---------------------------------------------------------------------------------------- */
int32_t dpft_stream_set(dpft_stream_t main_stream, int32_t n, dpft_stream_t* out);

/* ------------------------------------------------------------------------------------------
 * FPN glue + positional embedding
 * ---------------------------------------------------------------------------------------- */
/* lat[B,H,W,K] += nearest_upsample(top[B,TH,TW,K]) with src = min(floor(dst*in/out), in-1) */
int dpft_fpn_topdown_add_f32(float* lat, const float* top, int32_t B, int32_t H, int32_t W,
                             int32_t TH, int32_t TW, int32_t K, dpft_stream_t stream);
/* dtop[B,TH,TW,K] += sum of dlat over the pixels that map to each source pixel */
int dpft_fpn_topdown_add_bwd_f32(const float* dlat, float* dtop, int32_t B, int32_t H, int32_t W,
                                 int32_t TH, int32_t TW, int32_t K, dpft_stream_t stream);
/* x[B,H,W,K] += pos_x[W][K]; x += pos_y[H][K]  (two fp32 adds in the reference's order) */
int dpft_add_pos_f32(float* x, const float* pos_x, const float* pos_y, int32_t B, int32_t H,
                     int32_t W, int32_t K, dpft_stream_t stream);
/* One level of the neck's forward in two launches (src/dprt/models/necks/fpn.py:70-83 -> torchvision FeaturePyramidNetwork.forward;
 * src/dprt/models/embeddings/sinusoidal.py:107-108):
 *   lat = conv1x1(x, w, bias) [+ nearest_upsample(top[B,TH,TW,K])]          `d` = the 1x1 lateral conv's descriptor
 *   out = conv3x3(lat, w, bias) [+ pos_x[W][K]; + pos_y[H][K]]              `d` = the 3x3 output conv's descriptor
 * The adds ride in the convs' epilogues where a thin-channel kernel takes the shape (raw-input laterals C = 3 / 6 -> 16; the
 * 16 -> 16 3x3 convs): one pass over the level instead of two.  Everywhere else the function runs the conv followed by
 * dpft_fpn_topdown_add_f32 / dpft_add_pos_f32 -- the same arithmetic in the same order.  top / pos_x + pos_y may be NULL. */
int dpft_fpn_lateral_f32(const dpft_conv_desc* d, const float* x, const float* w, const float* bias, const float* top,
                         int32_t TH, int32_t TW, float* lat, void* workspace, dpft_stream_t stream);
int dpft_fpn_output_f32(const dpft_conv_desc* d, const float* lat, const float* w, const float* bias, const float* pos_x,
                        const float* pos_y, float* out, void* workspace, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Multi-scale deformable attention
 * ---------------------------------------------------------------------------------------- */
/* Operator-level drop-in for the MSDA extension (same tensor semantics):
 * value (N,S,M,D) f32; shapes (L,2) int64 [H,W]; lsi (L) int64; loc (N,Lq,M,L,P,2) f32 (x,y in
 * [0,1]); attn (N,Lq,M,L,P) f32; out (N,Lq,M*D). */
int dpft_msda_fwd_f32(const float* value, const int64_t* shapes, const int64_t* lsi,
                      const float* loc, const float* attn, float* out, int32_t N, int32_t S,
                      int32_t M, int32_t D, int32_t Lq, int32_t L, int32_t P, dpft_stream_t stream);
/* grad_value must be zero-filled by the caller (atomics accumulate into it). */
int dpft_msda_bwd_f32(const float* value, const int64_t* shapes, const int64_t* lsi,
                      const float* loc, const float* attn, const float* grad_out,
                      float* grad_value, float* grad_loc, float* grad_attn, int32_t N, int32_t S,
                      int32_t M, int32_t D, int32_t Lq, int32_t L, int32_t P, dpft_stream_t stream);
/* The same operator with typed storage (msda_typed.hip).  dtype: 0 fp32 | 1 IEEE half | 2 bf16 -- the type of value, attn,
 * out, grad_out, grad_value and grad_attn.  loc32 = 1: loc and grad_loc are fp32 whatever dtype is (what autocast hands
 * over); loc32 = 0: they have type dtype.  All arithmetic is fp32; every result is rounded to its type once, to nearest even.
 * Any M, D >= 1; the forward uses 16-byte accesses when D % 8 == 0 (D % 4 for fp32) and value / out are 16-byte aligned.
 * Backward: grad_value is summed by fp32 atomics in `workspace` (N*S*M*D floats; required for dtype != 0, ignored for 0,
 * where grad_value itself takes the sums) and rounded to dtype by a last pass.  The entry clears the sums itself on
 * `stream`: unlike dpft_msda_bwd_f32, nothing has to be zero-filled by the caller.  No allocation, no synchronisation. */
int dpft_msda_fwd_typed(const void* value, const int64_t* shapes, const int64_t* lsi, const void* loc,
                        const void* attn, void* out, int32_t N, int32_t S, int32_t M, int32_t D, int32_t Lq,
                        int32_t L, int32_t P, int32_t dtype, int32_t loc32, dpft_stream_t stream);
int dpft_msda_bwd_typed(const void* value, const int64_t* shapes, const int64_t* lsi, const void* loc,
                        const void* attn, const void* grad_out, void* grad_value, void* grad_loc, void* grad_attn,
                        float* workspace, int32_t N, int32_t S, int32_t M, int32_t D, int32_t Lq, int32_t L,
                        int32_t P, int32_t dtype, int32_t loc32, dpft_stream_t stream);

#define DPFT_MAX_LEVELS 8
typedef struct dpft_pyramid {
    const float* level[DPFT_MAX_LEVELS]; /* (B,H_l,W_l,C) NHWC, C = d_model */
    float* grad[DPFT_MAX_LEVELS];        /* same shapes, accumulated into (backward only) */
    int32_t H[DPFT_MAX_LEVELS], W[DPFT_MAX_LEVELS];
    int32_t L;
    /* grad_replicas[l] = R > 1: grad[l] is (R,B,H_l,W_l,C) and every query row adds into replica (row % R); the
     * caller sums the replicas.  Spreads the fp32 atomics of tiny levels (a 2x4 radar level would otherwise take
     * ~6000 serialized adds per address).  0 or 1 = plain buffer.  Honoured by dpft_xattn_ffn_train_bwd_f32. */
    int32_t grad_replicas[DPFT_MAX_LEVELS];
} dpft_pyramid;

/* Fused sample-then-project cross attention (C = M*D <= 64, L*P <= 32):
 *   samp[b,q,m,:C]  = sum_{l,p} attn * bilinear(level_l, ref + off/(W_l,H_l))     (raw features)
 *   mass[b,q,m]     = sum_{l,p} attn * (in-bounds bilinear weight mass)
 *   out[b,q,m*D+d]  = Wv[m*D+d,:] . samp[b,q,m,:] + bv[m*D+d] * mass[b,q,m]
 * which equals value_proj -> MSDA core of the reference (SURVEY App. C fusion identity).
 * ref (B,Q,2) (u,v); off (B,Q,M,L,P,2) raw sampling_offsets output; attn (B,Q,M,L,P) softmaxed.
 * samp (B,Q,M,C) and mass (B,Q,M) are saved for backward. */
int dpft_xattn_fwd_f32(const dpft_pyramid* pyr, const float* ref, const float* off,
                       const float* attn, const float* Wv, const float* bv, float* out,
                       float* samp, float* mass, int32_t B, int32_t Q, int32_t M, int32_t D,
                       int32_t P, dpft_stream_t stream);
/* grad_off/grad_attn/grad_ref are overwritten (grad_ref may be NULL); pyr->grad[] are accumulated
 * into with fp32 atomics (caller zero-fills).  Gradients of Wv/bv are tiny reductions of
 * grad_out (x) samp / mass and are left to the host framework. */
int dpft_xattn_bwd_f32(const dpft_pyramid* pyr, const float* ref, const float* off,
                       const float* attn, const float* Wv, const float* bv, const float* grad_out,
                       float* grad_off, float* grad_attn, float* grad_ref, int32_t B, int32_t Q,
                       int32_t M, int32_t D, int32_t P, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused inference decoder (eval mode, no autograd): d_model 16, 8 heads x head_dim 2, L*P <= 20, Mish
 * FFN (d_ffn 32), LayerNorm, 'linear' view reduction, 3-layer bias-free linear heads -- IMPFusion /
 * MPFusion / MLFusion / LinearDetectionHead at config/kradar*.json (src/dprt/models/fusers/mpfusion.py:122-229,
 * :416-514,:617-745, src/dprt/models/layers/ms_deform_attn.py:138-217, src/dprt/models/heads/detection.py:252-275).
 * Parameters are first PACKED (once per weight update) into lane-friendly transposed blobs; the forward is
 * then one call = 2 launches per iteration (self attention of all views | cross attention + FFN of all views +
 * view reduction + heads + next reference points).
 * ---------------------------------------------------------------------------------------- */
typedef struct dpft_decoder_view {   /* parameters of one MLFusion, torch layouts (out_features, in_features) */
    const float *in_proj_w, *in_proj_b, *out_proj_w, *out_proj_b, *norm1_w, *norm1_b;       /* self attention */
    const float *off_w, *off_b, *att_w, *att_b, *val_w, *val_b, *outp_w, *outp_b, *norm2_w, *norm2_b; /* MSDeformAttn */
    const float *ffn1_w, *ffn1_b, *ffn2_w, *ffn2_b, *norm3_w, *norm3_b;                       /* FFN */
} dpft_decoder_view;

int64_t dpft_decoder_packed_view_floats(void);   /* floats per packed MLFusion blob (training cross-attention kernels) */
int64_t dpft_decoder_packed_infer_floats(int32_t Q);  /* floats per packed MLFusion blob of the inference decoder */
int64_t dpft_decoder_packed_head_floats(void);   /* floats per packed reduction+head blob */
/* packed <- one MLFusion's parameters (L levels, P points of its MSDeformAttn) */
int dpft_decoder_pack_view_f32(const dpft_decoder_view* view, int32_t L, int32_t P, float* packed,
                               dpft_stream_t stream);
/* the same for all V views of a layer in one launch; packed = V consecutive blobs */
int dpft_decoder_pack_views_f32(const dpft_decoder_view* views, int32_t V, const int32_t* L, const int32_t* P, float* packed,
                                dpft_stream_t stream);
/* inference decoder's blob of one MLFusion = view `view_index` of one MPFusion layer: per-head in_proj rows with
 * 1/sqrt(d)*log2(e) folded into q, the offsets / logits matrix in the lanes' sample-slot order, the LDS image of the
 * cross-attention kernel, the input-independent part of the self-attention's q / k / v rows over pos (Q,16) =
 * query_embedding.weight (W pos_k + b; with query0 (Q,16) = the learned query table, non-NULL for the FIRST layer only,
 * the whole rows W (query0_k + pos_k) + b: that layer's input is a parameter),
 * and the hand-over to the NEXT layer's self-attention: next_in_proj_w[V] = in_proj_weight (48,16) of the next layer's
 * views (NULL for the last layer), composed with this layer's red_w = reduction_layer.weight (16, 16*V). */
int dpft_decoder_pack_infer_f32(const dpft_decoder_view* view, int32_t L, int32_t P, const float* red_w,
                                const float* const* next_in_proj_w, int32_t view_index, int32_t V,
                                const float* pos, const float* query0, int32_t Q, float* packed, dpft_stream_t stream);
/* packed <- reduction_layer.weight (16, 16*V) and head_w[4][3] = center/size/angle/class x (layers .0,.3,.6)
 * weights, passed as a flat array of 12 pointers */
int dpft_decoder_pack_head_f32(const float* red_w, const float* const* head_w, int32_t V, int32_t num_classes,
                               float* packed, dpft_stream_t stream);

/* work: caller-owned scratch of dpft_decoder_work_floats(B,Q,V) floats.  Final outputs go to
 * center/size/angle/cls: (B,Q,3) (B,Q,3) (B,Q,2) (B,Q,num_classes). */
typedef struct dpft_decoder_fwd {
    int32_t B, Q, V, iters, num_classes;
    int32_t n_points[4];
    const float* packed_views;           /* [iters][V] blobs of dpft_decoder_packed_infer_floats(Q) */
    const float* packed_heads;           /* [iters] blobs of dpft_decoder_packed_head_floats()     */
    const dpft_pyramid* pyr;             /* [V]                                          */
    const float* query0;                 /* fuser.query (Q,16)                           */
    const float* pos;                    /* fuser.query_embedding.weight (Q,16)          */
    const float* center0;                /* querent output (B,Q,3)                       */
    const float* T[4];                   /* label_to_X_t (B,4,4)                         */
    const float* P[4];                   /* label_to_X_p (B,p_rows,4)                    */
    const int64_t* shape[4];             /* X_shape[:, :2] contiguous (B,2) = (H, W)     */
    int32_t p_rows[4], has_t[4];         /* rows of P (3 or 4); transformation.any(): 1 / 0, or -1 = evaluated on the
                                            device (no host read-back of the matrices) */
    float* work;
    float *center, *size, *angle, *cls;
    const float* attn0;                  /* (V,Q,16) from dpft_decoder_attn0_f32, or NULL: the attention output of iteration 0
                                            (a constant of the weights) -- with it a forward is 2 * iters launches, not + 1 */
    int32_t shape_stride;                /* int64 elements between the rows of shape[v]: 0 = 2 (contiguous (B,2)); 3 reads the
                                            first two columns of the dataset's (B,3) X_shape rows in place */
} dpft_decoder_fwd;
/* iteration 0's self-attention output for one batch element -- its input is the learned query table (mpfusion.py:700-703),
 * so it depends on the weights only; call again after every weight change, like the pack functions */
int dpft_decoder_attn0_f32(const float* packed_views, const float* pos, int32_t Q, int32_t V, float* attn0,
                           dpft_stream_t stream);
int64_t dpft_decoder_work_floats(int32_t B, int32_t Q, int32_t V);
/* HOST code, no launch: the limits the decoder launches use -- out[0] queries per score block, out[1] key slices per score
 * block, out[2] query rows per cross-attention block, out[3] the largest Q that dpft_decoder_forward_f32 and
 * dpft_decoder_attn0_f32 admit (LDS of the score kernel); a larger Q is refused by both */
int dpft_decoder_limits(int32_t out[4]);
/* measurement aid: with DPFT_DEC_DBG=1024 in the environment the decoder kernels stamp a 100 MHz clock at their phase
 * boundaries; copies 2 kernels x 2048 blocks x 8 slots of uint64 (last launches) to dst (tools/decoder_stamps.py) */
int dpft_debug_decoder_stamps(uint64_t* dst);
int dpft_decoder_forward_f32(const dpft_decoder_fwd* d, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training path of the decoder's self-attention block, all V views of one MPFusion layer per call:
 *   y1[v] = LayerNorm1(x + dropout1(out_proj(MHA(x + pos, x + pos, x))))   with attention-probability dropout
 * = MLFusion.forward_self_attn, src/dprt/models/fusers/mpfusion.py:122-148 (nn.MultiheadAttention, d_model 16,
 * 8 heads).  Dropout masks are regenerated in the backward from (*seed, salt); p_drop = 0 disables them.
 * Saved for backward (caller-owned): lse (V,B,Q,8), attn (V,B,Q,16), zhat (V,B,Q,16), rstd (V,B,Q).
 * Backward: parameter gradients are ACCUMULATED into grads[v] (caller zero-fills); dx (V,B,Q,16) is the
 * gradient w.r.t. x through view v, dxp (V,B,Q,16) the part that also flows to pos; scratch holds
 * dpft_selfattn_train_scratch_floats(B,Q,V) floats.  x is (B,Q,16) with batch stride x_bstride (0 = broadcast).
 * ---------------------------------------------------------------------------------------- */
typedef struct dpft_sa_params {   /* torch layouts: in_proj (48,16), out_proj (16,16) */
    const float *in_w, *in_b, *out_w, *out_b, *n1_w, *n1_b;
} dpft_sa_params;
typedef struct dpft_sa_grads {
    float *in_w, *in_b, *out_w, *out_b, *n1_w, *n1_b;
} dpft_sa_grads;
int dpft_selfattn_train_fwd_f32(const dpft_sa_params* params, int32_t V, const float* x, int64_t x_bstride,
                                const float* pos, float p_drop, const int64_t* seed, int32_t salt,
                                float* y1, float* lse, float* attn, float* zhat, float* rstd,
                                int32_t B, int32_t Q, dpft_stream_t stream);
int dpft_selfattn_train_bwd_f32(const dpft_sa_params* params, int32_t V, const float* x, int64_t x_bstride,
                                const float* pos, float p_drop, const int64_t* seed, int32_t salt,
                                const float* dy1, const float* lse, const float* attn, const float* zhat,
                                const float* rstd, const dpft_sa_grads* grads, float* dx, float* dxp,
                                float* scratch, int32_t B, int32_t Q, dpft_stream_t stream);
int64_t dpft_selfattn_train_scratch_floats(int32_t B, int32_t Q, int32_t V);
/* host only, no launch: the compiled tile form (queries / keys per wave: 1, 2, 3, 4, 5, 6 or 8; a block holds four waves)
 * and the dynamic LDS bytes that the forward, the backward over queries and the backward over keys / values -- in that
 * order -- use for these sizes, from the code the two launch functions read (the DPFT_SA_QW_FWD / DPFT_SA_QW_BWD /
 * DPFT_SA_KW tuning variables included).  Same size checks as the launches. */
int dpft_selfattn_train_tiles(int32_t B, int32_t Q, int32_t V, int32_t qw[3], int64_t lds_bytes[3]);

/* ------------------------------------------------------------------------------------------
 * Training path of the decoder's deformable cross-attention + FFN block, all V views of one MPFusion layer:
 *   y2 = LayerNorm2(y1 + dropout2(output_proj(MSDeformAttn(y1 + pos, ref, pyramid))))
 *   y3 = LayerNorm3(y2 + dropout4(ffn2(dropout3(Mish(ffn1(y2))))))
 * = MLFusion.forward_cross_attn + forward_ffn, src/dprt/models/fusers/mpfusion.py:150-229 and
 * src/dprt/models/layers/ms_deform_attn.py:138-217.  `views` are the torch-layout parameters, `packed` the V
 * blobs made from them by dpft_decoder_pack_view_f32 (the caller re-packs after every weight update).
 * y1, y3, dy3, dy1, dqp are (V,B,Q,16); ref/dref (V,B,Q,2); pos (Q,16).
 * Forward: `saved` (V,B*Q,dpft_xattn_ffn_train_saved_floats()) or NULL receives what the backward would otherwise have to
 * gather again (the attention-weighted sampled features and in-bounds masses of every head).
 * Backward: recomputes the ALU-only part of the row's forward (takes the gathered part from `saved`; NULL = gathers
 * again), adds the pyramid gradients into pyr[v].grad[] (caller zero-fills) and writes the per-row factors of the
 * parameter gradients into rows (V,B*Q,dpft_xattn_ffn_train_row_floats()); the column layout is documented at the top
 * of dpft_amd/csrc/decoder_train_x.hip (XR_*) and consumed by dpft_amd/models/fusers/train_fused.py.
 * Pyramid gradients: `scratch` (V,B*Q,dpft_xattn_ffn_train_scratch_floats()) or NULL.  With it, maps of at most 2048
 * pixels whose gradient buffer is not replicated (grad_replicas <= 1) are scattered through an LDS image of the map by a
 * second launch (one fp32 atomic per touched element and query chunk instead of one per sample corner); larger maps, and
 * every map when scratch is NULL, take one fp32 atomic per sample corner and channel.  Both forms add the same terms;
 * only the order of the fp32 additions differs.
 * ---------------------------------------------------------------------------------------- */
int64_t dpft_xattn_ffn_train_row_floats(void);
int64_t dpft_xattn_ffn_train_saved_floats(void);
int64_t dpft_xattn_ffn_train_scratch_floats(void);
int dpft_xattn_ffn_train_fwd_f32(const dpft_pyramid* pyr, const dpft_decoder_view* views, const float* packed,
                                 int32_t V, const int32_t* n_points, const float* y1, const float* pos,
                                 const float* ref, float p_drop, const int64_t* seed, int32_t salt, float* y3,
                                 float* saved, int32_t B, int32_t Q, dpft_stream_t stream);
int dpft_xattn_ffn_train_bwd_f32(const dpft_pyramid* pyr, const dpft_decoder_view* views, const float* packed,
                                 int32_t V, const int32_t* n_points, const float* y1, const float* pos,
                                 const float* ref, float p_drop, const int64_t* seed, int32_t salt,
                                 const float* saved, const float* dy3, float* dy1, float* dqp, float* dref,
                                 float* rows, float* scratch, int32_t B, int32_t Q, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training path of the decoder's view reduction + detection head + next reference points (one layer):
 *   x = reduction_layer(cat_v y3[v]);  out_g = act_g(MLP_g(x));  center = out_center + prev_center;
 *   refs[v] = reference point of `center` in view v (input of the NEXT layer's cross attention)
 * = MPFusion 'linear' reduction (src/dprt/models/fusers/mpfusion.py:416-514), LinearDetectionHead
 * (src/dprt/models/heads/detection.py:252-275) and IMPFusion.get_reference_points (mpfusion.py:617-696).
 * `packed` comes from dpft_decoder_pack_head_f32.  y3 == NULL: only refs of prev_center are computed.
 * Backward: NULL gradient inputs mean "no gradient"; rows (B*Q, dpft_head_train_row_floats()) receives the
 * per-row factors of the weight gradients (columns HR_* in dpft_amd/csrc/decoder_train_h.hip).
 * ---------------------------------------------------------------------------------------- */
typedef struct dpft_head_train {
    const float* y3;               /* (V,B,Q,16) */
    const float* packed;           /* dpft_decoder_packed_head_floats() floats */
    const float* red_w;            /* reduction_layer.weight (16, 16*V) */
    const float* head_w[4][3];     /* center/size/angle/class x layers .0,.3,.6 (torch layouts) */
    const float* prev_center;      /* (B,Q,3) */
    const float* T[4];             /* (B,4,4) per view (may be NULL when has_t == 0) */
    const float* P[4];             /* (B,p_rows,4) */
    const int64_t* shape[4];       /* (B,2) = (H, W) */
    int32_t p_rows[4], has_t[4];
    int32_t num_classes;
    float *x, *center, *size, *angle, *cls;      /* forward outputs (B,Q,16) (B,Q,3) (B,Q,3) (B,Q,2) (B,Q,ncls) */
    float* refs;                                   /* (V,B,Q,2) or NULL */
    const float *dx, *dcenter, *dsize, *dangle, *dcls, *drefs;   /* backward inputs, any may be NULL */
    float *dy3, *dcenter_prev, *rows;              /* backward outputs */
    int32_t shape_stride;                          /* int64 elements between the rows of shape[v]; 0 = 2 */
} dpft_head_train;
int64_t dpft_head_train_row_floats(void);
int dpft_head_train_fwd_f32(const dpft_head_train* h, int32_t B, int32_t Q, int32_t V, dpft_stream_t stream);
int dpft_head_train_bwd_f32(const dpft_head_train* h, int32_t B, int32_t Q, int32_t V, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Backward of the reference points of a center that was NOT made by a head: the querent's output when it is learned
 * (LearnableQueries, src/dprt/models/queries/learnable.py; the forward is dpft_head_train_fwd_f32 with y3 == NULL).
 *   dcenter_prev[b][q] = sum_v  d refs[v][b][q] / d prev_center[b][q] ^T  drefs[v][b][q]
 * Reads of `h`: prev_center (B,Q,3), drefs (V,B,Q,2), T / P / p_rows / shape / shape_stride / has_t; writes dcenter_prev
 * (B,Q,3).  y3 must be NULL.  The rule is the one dpft_head_train_bwd_f32 applies to the center it makes, conventions
 * included: a coordinate outside the clip [0,1] passes no gradient; w == 0 passes the gradient of the undivided
 * coordinates; a coordinate exactly on 0 or 1 passes it (as torch.clip does); at r == 0 (the view's origin) the view
 * adds nothing; at rho == 0 (its vertical axis) only the range term remains, azimuth and elevation add exactly zero.
 * Elsewhere d elevation / d t = (180 / pi) / r^2 * (-tz tx / rho, -tz ty / rho, rho), which has no difference of nearly
 * equal terms and keeps its digits up to the axis.  Views are summed in index order.
 * ---------------------------------------------------------------------------------------- */
int dpft_ref_points_bwd_f32(const dpft_head_train* h, int32_t B, int32_t Q, int32_t V, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Learned query points (LearnableQueries.forward, src/dprt/models/queries/learnable.py:103-128): the (Q,3) parameter
 * repeated over the batch and transformed, center[b][q] = f(queries[q]), with f by `mode`: the identity, or Spher2Cart
 * (src/dprt/models/utils/transformations.py:212-281) of (r, phi, roh) in radians or degrees:
 *   (r cos(phi) cos(roh), r sin(phi) cos(roh), r sin(roh))
 * Backward: dqueries[q] = J_f(queries[q])^T sum_b dcenter[b][q]; the batch is summed by one thread, b ascending, so the
 * result is the same bits on every call (no atomics).  queries, dqueries (Q,3); center, dcenter (B,Q,3); B*Q*3 < 2^31.
 * ---------------------------------------------------------------------------------------- */
#define DPFT_QUERY_IDENTITY 0
#define DPFT_QUERY_SPHER2CART_RAD 1
#define DPFT_QUERY_SPHER2CART_DEG 2
int dpft_query_center_fwd_f32(const float* queries, int32_t mode, float* center, int32_t B, int32_t Q,
                              dpft_stream_t stream);
int dpft_query_center_bwd_f32(const float* dcenter, const float* queries, int32_t mode, float* dqueries, int32_t B,
                              int32_t Q, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Weight gradients of the fused training decoder from the per-row factor matrices its backward kernels write:
 *   out[g][out_off + a * n_b + b] = sum_r rows[g][r][col_a + a] * rows[g][r][col_b + b]     (a < n_a, b < n_b)
 * col_b < 0 (with n_b == 1): column sums of the a-columns.  rows (G,R,W); specs is a HOST array of <= 40 entries;
 * one launch for all specs and groups, fixed summation order.  Replaces the bmm / einsum / sum launches of
 * dpft_amd/models/fusers/train_fused.py (torch -> Tensile kernels) on the training step.
 * ---------------------------------------------------------------------------------------- */
typedef struct dpft_outer_spec {
    int32_t col_a, n_a, col_b, n_b;
    int64_t out_off;
} dpft_outer_spec;
int dpft_rows_outer_f32(const float* rows, int32_t G, int32_t R, int32_t W, const dpft_outer_spec* specs,
                        int32_t n_specs, float* out, int64_t out_gstride, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Up to DPFT_MEMOPS_MAX device-to-device copies / zero fills (src == NULL) in ONE launch: the host glue's small per-step
 * tensor copies and clears (static inputs of a replayed decoder graph, static-address plan inputs, reducer clears) -- the
 * reference's counterparts are Tensor.copy_ / zero_ calls of its training loop (src/dprt/training/trainer.py:107-150).
 * Pointers 4-byte aligned, sizes multiples of 4 bytes (16-byte accesses when both pointers allow); ops is a HOST array.
 * ---------------------------------------------------------------------------------------- */
#define DPFT_MEMOPS_MAX 16
typedef struct dpft_memop {
    void* dst;
    const void* src;      /* NULL = zero fill */
    uint64_t bytes;
} dpft_memop;
int dpft_memops(int32_t n, const dpft_memop* ops, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * dst[i] (+)= sum_s sum_{l < n_lead_s} src_s[l * inner + i], i < inner: leading-axis sums of the training decoder's backward in
 * one launch, fixed summation order (table order, leading index ascending).  The reference's counterparts are the implicit
 * sums of autograd (expand / repeat backward, gradient accumulation of a parameter with several uses:
 * src/dprt/models/fusers/mpfusion.py:601-668 uses query_embedding.weight in every layer).  srcs is a HOST array.
 * ---------------------------------------------------------------------------------------- */
#define DPFT_SUM_SRCS_MAX 16
typedef struct dpft_sum_src {
    const float* src;
    int32_t n_lead;
} dpft_sum_src;
int dpft_sum_leading_f32(int32_t n_src, const dpft_sum_src* srcs, int64_t inner, float* dst, int32_t accumulate,
                         dpft_stream_t stream);

/* dst_i[k] += src_i[k] (fp32) for the n entries of a DEVICE-resident dpft_memop table (bytes = 4 * elements), one launch:
 * gradient accumulation of many small parameters (autograd's AccumulateGrad of the reference's training loop,
 * src/dprt/training/trainer.py:134-141).  The table may be written after the launch has been CAPTURED in a hipGraph. */
int dpft_add_many_f32(int32_t n, const dpft_memop* table_device, dpft_stream_t stream);

/* *ptrs[i] += increment for n <= DPFT_I64_PTRS_MAX int64 device scalars in one launch (ptrs: HOST array): the
 * num_batches_tracked counters a train-mode BatchNorm forward bumps (torch.nn.BatchNorm2d; the reference's backbones are
 * torchvision ResNets, src/dprt/models/backbones/resnet.py:120-176). */
#define DPFT_I64_PTRS_MAX 256
int dpft_i64_add_many(int32_t n, int64_t* const* ptrs, int64_t increment, dpft_stream_t stream);

/* Dropout seed of the fused training decoder: *snap = *state; *state += increment (one launch, capturable).  The reference
 * draws its dropout masks from torch's generator (nn.Dropout in src/dprt/models/fusers/mpfusion.py:95-119). */
int dpft_seed_advance(int64_t* state, int64_t* snap, int64_t increment, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Matcher cost helper: GIoU3D of yaw-only boxes, (B,N) predictions x (B,Mg) targets.
 * boxes are (x,y,z,l,w,h,yaw) rows of 7 floats; out (B,N,Mg).
 * ---------------------------------------------------------------------------------------- */
int dpft_giou3d_yaw_f32(const float* pred, const float* gt, float* out, int32_t B, int32_t N,
                        int32_t Mg, dpft_stream_t stream);

/* Per-sample label tensors (host arrays of B device pointers: gt_center (m,3), gt_size (m,3), gt_angle (m,2), gt_class (m,C)
 * one-hot, fp32 contiguous; counts_host[b] = m) -> the padded batch tensors the matcher / loss / metric kernels read:
 * gt_box (B,Mmax,8) = center | size | angle, gt_onehot (B,Mmax,C), gt_id (B,Mmax) = argmax(gt_class), counts (B).
 * Replaces the per-sample decollate of src/dprt/training/assigner.py:92-111 / loss.py:524-541 (B <= 32 per call). */
int dpft_pack_targets_f32(const float* const* center, const float* const* size, const float* const* angle,
                          const float* const* cls, const int32_t* counts_host, int32_t B, int32_t Mmax, int32_t C,
                          float* gt_box, float* gt_onehot, int32_t* gt_id, int32_t* counts, dpft_stream_t stream);

/* Whole matcher cost (src/dprt/training/assigner.py:113-132) in one launch:
 * cost[b,n,j] = w0*(-cls[b,n,gt_id[b,j]]) + w1*L1(center) + w2*L1(size) + w3*L1(angle) - w4*GIoU3D, 0 for j >= counts[b].
 * gt_box (B,Mmax,8) = center | size | angle(2); weights5 is a HOST array. */
int dpft_match_cost_f32(const float* cls, const float* center, const float* size, const float* angle,
                        const float* gt_box, const int32_t* gt_id, const int32_t* counts,
                        const float* weights5, float* cost, int32_t B, int32_t N, int32_t Mmax, int32_t C,
                        dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * HOST function (no launch): the assignments of a batch, cost (B,N,Mmax) fp32 in host memory as dpft_match_cost_f32 wrote it,
 * sample b restricted to its first counts[b] targets.  match (B,Mmax,2) int32 = (query, target) pairs by ascending query
 * index, -1 padded; n_matched[b] = min(N, counts[b]).  = scipy.optimize.linear_sum_assignment per sample
 * (src/dprt/training/loss.py:305 through the assigner; scipy is third-party: its published algorithm -- Crouse 2016, shortest
 * augmenting paths, double precision -- restated in dpft_amd/csrc/cabi.cpp).  Non-finite or infeasible costs are an error.
 * ---------------------------------------------------------------------------------------- */
int dpft_lsap_batch_f32(const float* cost, int32_t B, int32_t N, int32_t Mmax, const int32_t* counts, int32_t* match,
                        int32_t* n_matched);
/* The host window of a training step in one call (round 5): dpft_lsap_batch_f32 on the read-back cost matrices -> upload of
 * assignments | matched counts from the caller's page-locked `packed_host` into `packed_dev` (both (B * Mmax * 2 + B) int32) ->
 * dpft_set_loss_fwd_total_f32 -> and, when dcls is not NULL, dpft_set_loss_bwd_f32 with d total / d term = sel straight into
 * (dcls, dcenter, dsize, dangle).  Replaces training/loss.py:296-373 + the `loss.backward()` hop into the head outputs between the
 * matcher's sync and the decoder's backward. */
int dpft_assign_loss_f32(const float* cost_host, const int32_t* counts_host, int32_t* packed_host, int32_t* packed_dev,
                         const float* cls, const float* center, const float* size, const float* angle, const float* gt_box,
                         const float* gt_onehot, const float* weights5, float alpha, const float* sel, float* scratch,
                         float* losses5, float* total, float* dcls, float* dcenter, float* dsize, float* dangle, int32_t B,
                         int32_t N, int32_t Mmax, int32_t C, dpft_stream_t stream);

/* The same assignments ON THE DEVICE (round 5; dpft_amd/csrc/lsap.hip): one wavefront per sample runs the step sequence of
 * dpft_lsap_batch_f32 (double precision duals, scipy's tie rule as an associative reduction over the 64 lanes) on the cost
 * matrices dpft_match_cost_f32 left in HBM: cost (B,N,Mmax), counts (B), match (B,Mmax,2), n_matched (B) all DEVICE memory; the
 * same pairs in the same order as the host function.  A kernel cannot return an error: status (one int32 in device or
 * page-locked host memory, zero before the first call, may be NULL) receives 1 + b for a non-finite entry / 0x10000 + b for an
 * infeasible problem / 0x20000 + b for counts[b] > Mmax of sample b, and that sample gets no pairs.  With it the training step has no host round trip between the
 * matcher and the criterion (src/dprt/training/loss.py:296-373: scipy on a .cpu() copy per sample). */
int dpft_lsap_batch_dev_f32(const float* cost, const int32_t* counts, int32_t* match, int32_t* n_matched, int32_t* status,
                            int32_t B, int32_t N, int32_t Mmax, dpft_stream_t stream);
/* dpft_assign_loss_f32 without the host: dpft_lsap_batch_dev_f32 -> dpft_set_loss_fwd_total_f32 -> (dcls != NULL)
 * dpft_set_loss_bwd_f32, three launches from one call.  packed_dev (B * Mmax * 2 + B) int32 = assignments | matched counts. */
int dpft_assign_loss_dev_f32(const float* cost, const int32_t* counts, int32_t* packed_dev, int32_t* status, const float* cls,
                             const float* center, const float* size, const float* angle, const float* gt_box,
                             const float* gt_onehot, const float* weights5, float alpha, const float* sel, float* scratch,
                             float* losses5, float* total, float* dcls, float* dcenter, float* dsize, float* dangle, int32_t B,
                             int32_t N, int32_t Mmax, int32_t C, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SetCriterion + batch reduction 'mean' (src/dprt/training/loss.py:17-60 focal loss with the raw-logit p_t,
 * :176-373 criterion, :486-564 weighting / reduction) for given assignments.
 * losses5 = batch-reduced, weighted (total_class, object_class, center, size, angle); match (B,Mmax,2) int32 =
 * (query, target) pairs in assignment order; weights5 (HOST array) in the same term order; gout5 (DEVICE) = upstream
 * gradient per term.  The backward writes d(sum_k gout5[k]*losses5[k]) / d{cls,center,size,angle}.
 * ---------------------------------------------------------------------------------------- */
int dpft_set_loss_fwd_f32(const float* cls, const float* center, const float* size, const float* angle,
                          const float* gt_box, const float* gt_onehot, const int32_t* match,
                          const int32_t* counts, const float* weights5, float alpha, float* losses5,
                          int32_t B, int32_t N, int32_t Mmax, int32_t C, dpft_stream_t stream);
/* The same forward in ONE launch without a cleared output, plus total = sum_k sel[k] * losses5[k] (sel: DEVICE, 5 floats -- the
 * configured terms; the reference sums them in src/dprt/training/loss.py:556-562): per-block partial sums in `scratch`
 * (dpft_set_loss_scratch_floats(B, N) floats, ZERO when first handed over, left zero), added in block order by the block that
 * draws the last ticket. */
int64_t dpft_set_loss_scratch_floats(int32_t B, int32_t N);
int dpft_set_loss_fwd_total_f32(const float* cls, const float* center, const float* size, const float* angle,
                                const float* gt_box, const float* gt_onehot, const int32_t* match,
                                const int32_t* counts, const float* weights5, float alpha, const float* sel,
                                float* scratch, float* losses5, float* total, int32_t B, int32_t N, int32_t Mmax,
                                int32_t C, dpft_stream_t stream);
int dpft_set_loss_bwd_f32(const float* cls, const float* center, const float* size, const float* angle,
                          const float* gt_box, const float* gt_onehot, const int32_t* match,
                          const int32_t* counts, const float* weights5, float alpha, const float* gout5,
                          float* dcls, float* dcenter, float* dsize, float* dangle, int32_t B, int32_t N,
                          int32_t Mmax, int32_t C, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Deep supervision (train.aux_loss): matcher cost, assignment, criterion and gradient over L supervised outputs ("layers";
 * layer 0 = the final decoder iteration, layer 1 + i = iteration i) with the launches of one output.  The layers are separate
 * allocations (a decoder graph's static output / gradient buffers): `layers` is a HOST array of L entries whose pointers
 * travel by value in the kernel arguments -- no stacking copy, no table upload.  Targets are shared: pseudo-sample
 * s = l * B + b reads gt_*[b].  Per-query and per-pair arithmetic are the __device__ functions the single-output kernels
 * call (csrc/misc.hip: match_cost_entry, set_loss_point), so entry [l] of every result has the bits of the single-output
 * entry on layer l's tensors.  Refused with a message: L < 1 or L > DPFT_LOSS_MAX_LAYERS, a null output, some but not all
 * gradient pointers of a layer, a negative or non-finite weight (dpft_loss_layers_check, called first by every entry).
 * ---------------------------------------------------------------------------------------- */
#define DPFT_LOSS_MAX_LAYERS 8
typedef struct dpft_loss_layer {
    const float *cls, *center, *size, *angle; /* (B,N,C) (B,N,3) (B,N,3) (B,N,2) DEVICE, contiguous */
    float *dcls, *dcenter, *dsize, *dangle;   /* gradient buffers of the same shapes: all four or all NULL */
    float weight;                             /* of this layer's total in `total` and in its gradient */
} dpft_loss_layer_t;
int dpft_loss_layers_check(const dpft_loss_layer_t* layers, int32_t L);
/* cost (L,B,N,Mmax): entry [l] = dpft_match_cost_f32 on layer l; counts_tiled (L*B) int32 = counts repeated per layer, so
 * that dpft_lsap_batch_dev_f32 / dpft_lsap_batch_f32 run unchanged on L*B pseudo-samples.  One launch, grid (.., L). */
int dpft_match_cost_layers_f32(const dpft_loss_layer_t* layers, int32_t L, const float* gt_box, const int32_t* gt_id,
                               const int32_t* counts, const float* weights5, float* cost, int32_t* counts_tiled, int32_t B,
                               int32_t N, int32_t Mmax, int32_t C, dpft_stream_t stream);
/* match (L,B,Mmax,2), counts (L,B) = the assignment of the L*B pseudo-samples.  One launch, grid (blocks of a layer, L);
 * scratch: dpft_set_loss_layers_scratch_floats(L,B,N) floats, zero when first handed over, left zero.  The block that draws
 * the last ticket writes losses (L,5): row l = the five weighted batch-mean terms of layer l (block order, WITHOUT the layer
 * weight: the bits of dpft_set_loss_fwd_total_f32 on layer l), layer_totals (L) = weight_l * sum_k sel[k] * losses[l,k]
 * (k ascending) and total = their sum in layer order. */
int64_t dpft_set_loss_layers_scratch_floats(int32_t L, int32_t B, int32_t N);
int dpft_set_loss_layers_fwd_total_f32(const dpft_loss_layer_t* layers, int32_t L, const float* gt_box, const float* gt_onehot,
                                       const int32_t* match, const int32_t* counts, const float* weights5, float alpha,
                                       const float* sel, float* scratch, float* losses, float* layer_totals, float* total,
                                       int32_t B, int32_t N, int32_t Mmax, int32_t C, dpft_stream_t stream);
/* d (gout * total) / d (cls, center, size, angle) of every layer that names gradient buffers (at least one must), one launch:
 * term k of layer l has the factor (weight_l * gout * sel[k]) * weights5[k] / B, i.e. dpft_set_loss_bwd_f32 with
 * gout5 = (weight_l * gout) * sel.  gout: DEVICE scalar, NULL = 1. */
int dpft_set_loss_layers_bwd_f32(const dpft_loss_layer_t* layers, int32_t L, const float* gt_box, const float* gt_onehot,
                                 const int32_t* match, const int32_t* counts, const float* weights5, float alpha,
                                 const float* sel, const float* gout, int32_t B, int32_t N, int32_t Mmax, int32_t C,
                                 dpft_stream_t stream);
/* The layered twins of dpft_assign_loss_dev_f32 / dpft_assign_loss_f32: assignment of the L*B pseudo-samples
 * (dpft_lsap_batch_dev_f32 on cost (L,B,N,Mmax) with counts_tiled (L*B) DEVICE; respectively dpft_lsap_batch_f32 on the HOST
 * copy with counts_host (B) + one upload) -> dpft_set_loss_layers_fwd_total_f32 -> dpft_set_loss_layers_bwd_f32 (gout NULL)
 * when a layer names gradient buffers; three launches from one call.  packed_* : (L*B*Mmax*2 + L*B) int32 = assignments |
 * matched counts; layer 0's slices of both are contiguous.  Status codes as dpft_lsap_batch_dev_f32 with sample l * B + b. */
int dpft_assign_loss_layers_dev_f32(const float* cost, const int32_t* counts_tiled, int32_t* packed_dev, int32_t* status,
                                    const dpft_loss_layer_t* layers, int32_t L, const float* gt_box, const float* gt_onehot,
                                    const float* weights5, float alpha, const float* sel, float* scratch, float* losses,
                                    float* layer_totals, float* total, int32_t B, int32_t N, int32_t Mmax, int32_t C,
                                    dpft_stream_t stream);
int dpft_assign_loss_layers_f32(const float* cost_host, const int32_t* counts_host, int32_t* packed_host, int32_t* packed_dev,
                                const dpft_loss_layer_t* layers, int32_t L, const float* gt_box, const float* gt_onehot,
                                const float* weights5, float alpha, const float* sel, float* scratch, float* losses,
                                float* layer_totals, float* total, int32_t B, int32_t N, int32_t Mmax, int32_t C,
                                dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Optional sixth criterion term (train.loss_weights["giou"]; the reference's GIoULoss, src/dprt/training/loss.py:111-173, needs
 * pytorch3d and has no backward): the differentiable GIoU3D of the matched pairs,
 *   term = w_giou / B * sum_b 1 / counts[b] * sum_k (1 - G(pred[b, i_k], gt[b, j_k])) / 2,      (i_k, j_k) = match[b, k]
 * match (B,Mmax,2) and counts (B) as the assignment entries leave them.  G = the matcher's yaw-box GIoU3D in fp64 with
 * union = v1 + v2 - vol always (the textbook value for disjoint boxes, not the reference's constant -1) and
 * yaw = atan2(sin, cos) in fp64, differentiated through; an invalid box (min(lw, lh, wh) / 2 <= 1e-4 or a size <= 0) gives
 * G = -1 and no gradient.  One workgroup, fp64 sums in a fixed order: repeated launches give the same bits.
 * fwd: term (1 float) and, when total_in / total_out (device scalars, both or neither) are given, total_out = total_in + term;
 *      g_pairs (B,Mmax), may be NULL: G per pair slot (0 in empty slots).
 * bwd: d (gout * term) / d (center, size, angle); gout = DEVICE scalar, NULL = 1.  accumulate = 0: all B * N rows are written
 *      (zeros for unmatched queries); accumulate = 1: the fp32-rounded gradient is added to the matched rows only (bit-equal
 *      to the write form followed by an fp32 add).
 * ---------------------------------------------------------------------------------------- */
int dpft_giou_loss_fwd_f32(const float* center, const float* size, const float* angle, const float* gt_box,
                           const int32_t* match, const int32_t* counts, float w_giou, const float* total_in, float* term,
                           float* total_out, float* g_pairs, int32_t B, int32_t N, int32_t Mmax, dpft_stream_t stream);
int dpft_giou_loss_bwd_f32(const float* center, const float* size, const float* angle, const float* gt_box,
                           const int32_t* match, const int32_t* counts, float w_giou, const float* gout, float* dcenter,
                           float* dsize, float* dangle, int32_t accumulate, int32_t B, int32_t N, int32_t Mmax,
                           dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Input preprocessing on the device (the reference does it per sample in DataLoader workers):
 * camera frame resize = torchvision.transforms.functional.resize(bilinear, no antialias) on the HWC frame
 * (src/dprt/datasets/kradar/dataset.py:319-341), from fp32 or straight from the decoded u8 bytes; radar map scaling
 * (v - in_lo) / (in_hi - in_lo) * (out_hi - out_lo) + out_lo clipped to [out_lo, out_hi] (dataset.py:295-317 with
 * in = (min_power, max_power) = (100, 200), out = (0, 255)).  NHWC in and out.
 * ---------------------------------------------------------------------------------------- */
int dpft_resize_bilinear_nhwc_f32(const float* src, float* dst, int32_t B, int32_t Hs, int32_t Ws, int32_t Hd,
                                  int32_t Wd, int32_t C, dpft_stream_t stream);
int dpft_resize_bilinear_nhwc_u8(const uint8_t* src, float* dst, int32_t B, int32_t Hs, int32_t Ws, int32_t Hd,
                                 int32_t Wd, int32_t C, dpft_stream_t stream);
int dpft_scale_clip_f32(const float* x, float* y, int64_t n, float in_lo, float in_hi, float out_lo,
                        float out_hi, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training augmentation on the device (optional, "train.augment"; DESIGN.md section 3 "Training augmentation" states the
 * coordinate contract): one horizontal flip per sample applied to every view and to the labels, a camera zoom / shift about
 * the canvas centre, a photometric step on the camera frame and a gain on the radar maps.  The parameters are drawn on the
 * HOST and passed as a host array of B samples; the entries copy them into the kernel arguments, DPFT_AUGMENT_CHUNK samples
 * per launch (B above that: one launch per chunk) -- no device copy, no host wait, no allocation, stream-ordered.
 *
 * dpft_augment_sample: canvas coordinates in units of the canvas (u / W, v / H, edge convention):
 *   u' = a u + bu,  v' = s v + bv;  s > 0 the zoom, a = s (a = -s and flip = 1 on a flipped sample, with bu already mirrored,
 *   bu -> 1 - bu);  radar maps take only the flip.  gain[c] v + offset clipped to [0, 255] is the photometric step (all gains
 *   1 and offset 0: skipped), delta_db is added to the radar maps before their scaling.
 *
 * camera: replaces the resize launch -- one thread per output pixel, C <= 4.  The centre of output pixel (x, y) goes through
 *   the inverse map to the source; a pixel whose source centre lies outside [0, Ws] x [0, Hs] is written as 0, inside taps
 *   clamp to the frame.  With s == 1, bv == 0 and bu == flip the result has the bits of the resize entries' output, or of that
 *   output mirrored along x.
 * radar: replaces dpft_scale_clip_f32 -- clip(((x + delta_db) - in_lo) / (in_hi - in_lo) * (out_hi - out_lo) + out_lo) read
 *   from the mirrored index of axis 2 of (B,H,W,C) on a flipped sample; scale = 0: the flip alone.  delta_db = 0 and no flip
 *   gives the bits of dpft_scale_clip_f32.
 * geometry: one launch per chunk for all views and labels, OUT OF PLACE (the inputs are left as they are).  Per view
 *   P' = M P diag(1,-1,1,1) and T' = F T F, F = diag(1,-1,1,1) (column negation and T' on flipped samples only; zeros keep
 *   their sign); M = identity but M[0,0] = a, M[0,2] = bu W, M[1,1] = s, M[1,2] = bv H with (H, W) read from the view's int64
 *   shape rows, on views with zoom = 1 (cameras); a = -1 / 1, bu W = W / 0 on the others.  Labels of a flipped sample:
 *   center y and angle sin negated.  labels may be NULL; a sample with rows = 0 may have null pointers.
 * ---------------------------------------------------------------------------------------- */
#define DPFT_AUGMENT_CHUNK 8
#define DPFT_AUGMENT_MAX_VIEWS 4
typedef struct dpft_augment_sample {
    float a, bu, s, bv;
    float gain[4];
    float offset;
    float delta_db;
    int32_t flip;
    int32_t pad;
} dpft_augment_sample;
typedef struct dpft_augment_view {
    const float* T;            /* (B,4,4) */
    const float* P;            /* (B,p_rows,4) */
    float* T_out;
    float* P_out;
    const int64_t* shape;      /* rows (H, W, ...) of shape_stride elements */
    int32_t shape_stride;
    int32_t p_rows;            /* 3 or 4 */
    int32_t zoom;              /* 1: the zoom / shift part of M acts on this view (cameras) */
    int32_t pad;
} dpft_augment_view;
typedef struct dpft_augment_labels {
    const float* center;       /* (rows,3) */
    const float* angle;        /* (rows,2) = [sin, cos] */
    float* center_out;
    float* angle_out;
    int32_t rows;
    int32_t pad;
} dpft_augment_labels;
int dpft_augment_camera_nhwc_f32(const float* src, float* dst, int32_t B, int32_t Hs, int32_t Ws, int32_t Hd, int32_t Wd,
                                 int32_t C, const dpft_augment_sample* samples, dpft_stream_t stream);
int dpft_augment_camera_nhwc_u8(const uint8_t* src, float* dst, int32_t B, int32_t Hs, int32_t Ws, int32_t Hd, int32_t Wd,
                                int32_t C, const dpft_augment_sample* samples, dpft_stream_t stream);
int dpft_augment_radar_nhwc_f32(const float* x, float* y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t scale,
                                float in_lo, float in_hi, float out_lo, float out_hi, const dpft_augment_sample* samples,
                                dpft_stream_t stream);
int dpft_augment_geometry_f32(const dpft_augment_view* views, int32_t V, const dpft_augment_labels* labels,
                              const dpft_augment_sample* samples, int32_t B, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Sensor degradation on the device (optional, "train.corrupt" and "evaluate.robustness"; DESIGN.md section 3 "Sensor
 * degradation").  Both launches work on PREPROCESSED inputs, out of place (dst != src), with the per-sample parameters as a
 * host array of B samples copied into the kernel arguments, DPFT_CORRUPT_CHUNK samples per launch -- no device copy, no host
 * wait, no allocation, stream-ordered.  A sample whose parameters are all neutral is copied bit for bit.
 *
 * Noise: v + noise * z, product and sum rounded separately, z = float(u0 + u1 + u2 + u3 - 131070) * (1 / 37837.2f) out of four
 *   16-bit uniforms (Irwin-Hall of order 4: unit variance, |z| < 3.47) that are a pure integer function of (key, view, element
 *   index within the sample): with mix(x) = the 32-bit multiply-xorshift mixer (x ^= x >> 16, x *= 0x7feb352d, x ^= x >> 15,
 *   x *= 0x846ca68b, x ^= x >> 16), lo / hi the halves of key,
 *     s0 = mix(lo ^ mix(hi ^ mix(view ^ 0x9e3779b9))),  s1 = mix(hi ^ mix(lo ^ mix(view ^ 0xc2b2ae35))),
 *     a = mix(index ^ s0),  b = mix(a ^ s1),  u = the 16-bit halves of a and b.  There is no device random state.
 *
 * camera (B,H,W,C <= 4), nominally in [0, 255]; per sample, in this order:
 *   1. Gaussian blur, separable (horizontal, then vertical), replicate border: radius = ceil(3 sigma) <= DPFT_CORRUPT_MAX_RADIUS
 *      (sigma in (0, 5]; sigma = 0 and radius = 0: no blur), half table w[0..radius] with w[0] + 2 sum w[k] = 1 (the caller
 *      normalises exp(-k^2 / 2 sigma^2) in double precision and rounds once).  A tiled LDS kernel: the tile and its halo are staged
 *      once per workgroup, both passes run out of LDS.
 *   2. haze: v + haze * (airlight[c] - v), haze in [0, 1], three roundings (haze = 0: skipped);
 *   3. noise (above), clamped to [0, 255] when noise > 0, index = (y W + x) C + c;
 *   4. erase: n_rects <= 4 rectangles [x0, x1) x [y0, y1) inside the frame (rect = x0, x1, y0, y1), each set to fill[c];
 *   5. off: the whole frame becomes 0.
 * radar (B,H,W,C <= 32), axis 2 = azimuth: noise on the channels of the bit mask `channels`, clamped to [lo, hi] when
 *   noise > 0; n_azimuth <= 4 bands [a0, a1) of axis 2 and n_rows <= 4 bands [r0, r1) of axis 1 are set to lo; off: 0.
 * limits (host only): out = tile height, tile width of the camera launch, DPFT_CORRUPT_MAX_RADIUS, DPFT_CORRUPT_CHUNK.
 * Refused (nothing is launched): sigma outside [0, 5], haze outside [0, 1], NaN or negative noise, C > 4 (camera), a rectangle
 *   or band outside the frame, weights that do not add up to 1, null pointers, dst == src.
 * ---------------------------------------------------------------------------------------- */
#define DPFT_CORRUPT_CHUNK 8
#define DPFT_CORRUPT_MAX_RADIUS 15
#define DPFT_CORRUPT_MAX_RECTS 4
#define DPFT_CORRUPT_MAX_BANDS 4
typedef struct dpft_corrupt_camera {
    uint64_t key;
    int32_t view;
    int32_t radius;
    float sigma;
    float w[DPFT_CORRUPT_MAX_RADIUS + 1];
    float haze;
    float airlight[4];
    float noise;
    int32_t n_rects;
    int32_t rect[DPFT_CORRUPT_MAX_RECTS][4];
    float fill[DPFT_CORRUPT_MAX_RECTS][4];
    int32_t off;
} dpft_corrupt_camera;
typedef struct dpft_corrupt_radar {
    uint64_t key;
    int32_t view;
    float noise;
    uint32_t channels;
    int32_t n_azimuth;
    int32_t azimuth[DPFT_CORRUPT_MAX_BANDS][2];
    int32_t n_rows;
    int32_t rows[DPFT_CORRUPT_MAX_BANDS][2];
    int32_t off;
    int32_t pad;
} dpft_corrupt_radar;
int dpft_corrupt_limits(int32_t out[4]);
int dpft_corrupt_camera_nhwc_f32(const float* src, float* dst, int32_t B, int32_t H, int32_t W, int32_t C,
                                 const dpft_corrupt_camera* samples, dpft_stream_t stream);
int dpft_corrupt_radar_nhwc_f32(const float* x, float* y, int32_t B, int32_t H, int32_t W, int32_t C, float lo, float hi,
                                const dpft_corrupt_radar* samples, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-step detection metrics of the reference's train / validation loops (src/dprt/training/trainer.py:134,
 * src/dprt/evaluation/metric.py): mAP3D (IoU threshold, nelem-point "interpolated" curve, :16-151) and mGIoU3D
 * (:154-253) of every sample, on padded targets.  out (B,2) = (mAP, mGIoU) per sample (the caller applies the batch
 * reduction); scratch holds 2*B*N*Mmax floats (IoU, GIoU of every pair).  N <= 1024, Mmax <= 256, C <= 16.
 * ---------------------------------------------------------------------------------------- */
int dpft_detection_metrics_f32(const float* cls, const float* center, const float* size, const float* angle,
                               const float* gt_box, const float* gt_onehot, const int32_t* counts,
                               float threshold, int32_t nelem, float* scratch, float* out, int32_t B,
                               int32_t N, int32_t Mmax, int32_t C, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Split-level AP_BEV / AP_3D accumulated on the device (dpft_amd/evaluation/dataset_ap.py states the definition).
 * A combination k < K (1 <= K <= 8) is an IoU kind (kinds[k]: 0 bev, 1 3d) and a threshold inside (0, 1); iou_thrs,
 * kinds and roi6 are HOST arrays (roi6 = xmin, xmax, ymin, ymax, zmin, zmax with strict inequalities, NULL = no filter).
 * update (two launches, no read-back): pairwise fp64 IoUs into scratch (dpft_dataset_ap_scratch_bytes), then per sample
 *   the detections (argmax class != 0, score >= min_score, centre inside the roi, score not NaN) in (score desc, query
 *   asc) order each take the best unassigned target of their class with IoU > threshold.  Every detection appends one
 *   16-byte record (int32 x 4: score bits, first_frame + b, query | class << 16, TP bit per combination) at a position
 *   reserved with one atomic on counters[0]; record order is arbitrary.  counters (32 int64, zero before the first
 *   update): [0] cursor, [1] queries dropped for a NaN score, [2] records refused for lack of capacity, [16 + c]
 *   ground-truth count of class c.  `reserved` = host-known upper bound of the cursor (sum of B * N of earlier updates):
 *   capacity - reserved >= B * N is required, and the kernel never writes at or past capacity.
 *   N <= 1024, Mmax <= 256, 2 <= C <= 16.  gt_box / gt_id / counts as dpft_pack_targets_f32 writes them.
 * finalize: records_sorted = the n_records records ordered by (class, score desc, frame asc, query asc), class_start
 *   (C + 1 int64, device) the first record of every class.  One workgroup per (class, combination): ap (C-1,K) =
 *   mean over r_i = i / R, i = 1..R (2 <= R <= 101), of max{precision(p) : recall(p) >= r_i} (NaN for a class without
 *   ground truth), npos (C-1), tp_total (C-1,K); all fp64.
 * ---------------------------------------------------------------------------------------- */
int64_t dpft_dataset_ap_scratch_bytes(int32_t B, int32_t N, int32_t Mmax);      /* -1 + dpft_last_error() when out of range */
int dpft_dataset_ap_update_f32(const float* cls, const float* center, const float* size, const float* angle,
                               const float* gt_box, const int32_t* gt_id, const int32_t* counts,
                               const double* iou_thrs, const int32_t* kinds, int32_t K, const float* roi6,
                               float min_score, void* scratch, void* records, int64_t capacity, int64_t reserved,
                               int64_t* counters, int32_t first_frame, int32_t B, int32_t N, int32_t Mmax,
                               int32_t C, dpft_stream_t stream);
int dpft_dataset_ap_finalize_f64(const void* records_sorted, int64_t n_records, const int64_t* class_start,
                                 const int64_t* counters, int32_t C, int32_t K, int32_t R, double* ap,
                                 double* npos, double* tp_total, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Split-level AP per scene-description group (evaluate.dataset_ap.groups; dpft_amd/evaluation/dataset_ap.py).  Group 0
 * is "all"; every selected axis s < n_axes (<= 3) adds axis_counts[s] (1..16) groups, one per entry of
 * axis_values[s * 16 + i], in this order; at most 32 groups.  axis_cols[s] is the axis's column of the frame's
 * description [road, time, weather].  A description value is truncated towards zero; a non-finite one, or one equal to
 * no entry, leaves the frame without a group on that axis.
 * update_groups: dpft_dataset_ap_update_f32 (same two launches, same records and counters) whose match pass also writes
 *   row frames_before + b of the frame store `frames` (frame_capacity rows of 18 int32: first_frame + b, group bitmask,
 *   ground-truth count of classes 0..15) -- no atomic; frame_capacity - frames_before >= B and B <= 64 are required.
 *   The descriptions travel by value: desc_types[b] (HOST array) = 0 fp32, 1 fp64, 2 int32, 3 int64 with desc_ptrs[b]
 *   (HOST array of DEVICE pointers to >= 3 elements, aligned to the element), or 4 = the three doubles desc_host[3 * b ..]
 *   (HOST).  axis_cols, axis_counts and axis_values (n_axes x 16 int32) are HOST arrays.
 * finalize_groups (two launches): record_groups (n_records uint32, device) = the group bitmask of every sorted record's
 *   frame; frames = the n_frames rows of the frame store in any order; axis_masks (HOST, n_axes) = the bits of every
 *   axis.  First nframes (G), npos (G,C-1) and bad[0] (frames without a group on some axis) as integer sums over the
 *   frame rows, then one workgroup per (group, class, combination): dpft_dataset_ap_finalize_f64 applied to the member
 *   records alone (rank = members so far), ap (G,C-1,K) and tp_total (G,C-1,K); all fp64, the bits of an ungrouped run
 *   over the group's frames.
 * ---------------------------------------------------------------------------------------- */
int dpft_dataset_ap_update_groups_f32(const float* cls, const float* center, const float* size, const float* angle,
                                      const float* gt_box, const int32_t* gt_id, const int32_t* counts,
                                      const double* iou_thrs, const int32_t* kinds, int32_t K, const float* roi6,
                                      float min_score, void* scratch, void* records, int64_t capacity, int64_t reserved,
                                      int64_t* counters, int32_t first_frame, int32_t B, int32_t N, int32_t Mmax,
                                      int32_t C, const void* const* desc_ptrs, const int32_t* desc_types,
                                      const double* desc_host, const int32_t* axis_cols, const int32_t* axis_counts,
                                      const int32_t* axis_values, int32_t n_axes, void* frames, int64_t frame_capacity,
                                      int64_t frames_before, dpft_stream_t stream);
int dpft_dataset_ap_finalize_groups_f64(const void* records_sorted, const uint32_t* record_groups, int64_t n_records,
                                        const int64_t* class_start, const void* frames, int64_t n_frames,
                                        const uint32_t* axis_masks, int32_t n_axes, int32_t G, int32_t C, int32_t K,
                                        int32_t R, double* ap, double* npos, double* tp_total, double* nframes,
                                        double* bad, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * True-positive errors beside the split-level AP (evaluate.dataset_ap.tp_errors; dpft_amd/evaluation/dataset_ap.py
 * states the definition).  ref_k < K is the reference combination; a TP of it is the (detection, target) pair the greedy
 * walk of dpft_dataset_ap_update_f32 makes for that combination.
 * update_tp / update_groups_tp: dpft_dataset_ap_update_f32 / _groups_f32 (same two launches, the same records, counters
 *   and frame rows) whose match pass also writes row `position of the record` of tp_errors (capacity rows of 4 int64,
 *   16-byte aligned, the capacity of `records`): for a TP of ref_k the errors ate = sqrt(dx^2 + dy^2), aze = |dz|,
 *   ase = 1 - P / (Vd + Vg - P) with P = min(l) min(w) min(h), aoe = atan2(|s1 c2 - c1 s2|, c1 c2 + s1 s2) on the
 *   hypot-normalised (sin, cos) pairs (fold_pi = 1: min(aoe, pi - aoe)), each in fp64 from the fp32 inputs and stored as
 *   rint(e * 2^32), half to even; zeros for every other record.  An error that is not finite or not below 2^20 in
 *   magnitude stores 2^52 and counts in counters[3].  The kernel never writes at or past capacity.
 * finalize_tp: tp_errors_sorted (n_records x 4 int64, 16-byte aligned) = the error rows in the order of records_sorted.
 *   One workgroup per class: T = running TP count of ref_k, S = running integer sums; the TP with count T serves the
 *   recall points floor((T-1) R / npos) < i <= min(floor(T R / npos), R) with S / 2^32 / T; tp_err (C-1,4) = mean of the
 *   served points i >= i_min (1 <= i_min <= R) in ascending i, NaN when none is served; tp_points (C-1) their count.
 * finalize_tp_groups: the same per (group, class) over the member records (record_groups as finalize_groups takes it),
 *   group_npos (G,C-1, device) = the npos finalize_groups wrote; tp_err (G,C-1,4), tp_points (G,C-1): the bits of an
 *   ungrouped run over the group's frames.  All outputs fp64.
 * ---------------------------------------------------------------------------------------- */
int dpft_dataset_ap_update_tp_f32(const float* cls, const float* center, const float* size, const float* angle,
                                  const float* gt_box, const int32_t* gt_id, const int32_t* counts,
                                  const double* iou_thrs, const int32_t* kinds, int32_t K, const float* roi6,
                                  float min_score, void* scratch, void* records, int64_t capacity, int64_t reserved,
                                  int64_t* counters, int32_t first_frame, int32_t B, int32_t N, int32_t Mmax,
                                  int32_t C, void* tp_errors, int32_t ref_k, int32_t fold_pi, dpft_stream_t stream);
int dpft_dataset_ap_update_groups_tp_f32(const float* cls, const float* center, const float* size, const float* angle,
                                         const float* gt_box, const int32_t* gt_id, const int32_t* counts,
                                         const double* iou_thrs, const int32_t* kinds, int32_t K, const float* roi6,
                                         float min_score, void* scratch, void* records, int64_t capacity,
                                         int64_t reserved, int64_t* counters, int32_t first_frame, int32_t B, int32_t N,
                                         int32_t Mmax, int32_t C, const void* const* desc_ptrs, const int32_t* desc_types,
                                         const double* desc_host, const int32_t* axis_cols, const int32_t* axis_counts,
                                         const int32_t* axis_values, int32_t n_axes, void* frames, int64_t frame_capacity,
                                         int64_t frames_before, void* tp_errors, int32_t ref_k, int32_t fold_pi,
                                         dpft_stream_t stream);
int dpft_dataset_ap_finalize_tp_f64(const void* records_sorted, const int64_t* tp_errors_sorted, int64_t n_records,
                                    const int64_t* class_start, const int64_t* counters, int32_t C, int32_t ref_k,
                                    int32_t R, int32_t i_min, double* tp_err, double* tp_points, dpft_stream_t stream);
int dpft_dataset_ap_finalize_tp_groups_f64(const void* records_sorted, const int64_t* tp_errors_sorted,
                                           const uint32_t* record_groups, int64_t n_records, const int64_t* class_start,
                                           const double* group_npos, int32_t G, int32_t C, int32_t ref_k, int32_t R,
                                           int32_t i_min, double* tp_err, double* tp_points, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * KITTI-protocol table beside the split-level AP (evaluate.dataset_ap.kitti; dpft_amd/evaluation/dataset_ap.py states
 * the protocol -- target-major two-pass matching, <= 41 score thresholds per class and combination -- and the two
 * one-bit reductions used here; one difficulty level, no don't-care regions, no neighbouring classes).
 * update_kitti: dpft_dataset_ap_update_f32 (same two launches, records, counters and capacity rule) whose match pass
 *   also sets, in the record's fourth word, bit 8 + k = pass-1 TP of combination k (targets in ascending index each take
 *   the first unassigned detection in (score desc, query asc) order with IoU > threshold and score >= 0) and bit 16 + k =
 *   pass-2 bit (the detections inserted in that order into a target-major largest-IoU matching, ties to the lower
 *   query; set when the insertion adds a matched target).  Bits 0..7 stay the TP bits of dpft_dataset_ap_update_f32.
 *   frames = NULL: without groups (desc_*, axis_*, n_axes, frame_capacity, frames_before are not read); otherwise the
 *   frame rows of dpft_dataset_ap_update_groups_f32.  tp_errors = NULL: without true-positive errors (ref_k, fold_pi are
 *   not read); otherwise the error rows of dpft_dataset_ap_update_tp_f32 (on the VOC matching of bits 0..7).
 * finalize_kitti: records_sorted / class_start / counters as dpft_dataset_ap_finalize_f64 takes them.  One workgroup per
 *   (class, combination): n1 = pass-1 bits, G = npos; the thresholds are the scores of the pass-1 TPs (descending) at the
 *   ranks the tool's fp64 sampling loop picks (cur = 0; rank i is skipped while (i + 2) / G - cur < cur - (i + 1) / G and
 *   i < n1 - 1; cur += 1 / 40.0 per pick); at threshold s, A = records with score >= s, tp = pass-2 bits among them,
 *   fp = A - tp, prec = tp / A, rec = tp / G.  Outputs fp64: prec, rec, tp, fp (C-1,K,41; zeros from nthr on),
 *   thresholds (C-1,K,41; NaN from nthr on), ap40 (C-1,K) = mean of the suffix maximum of prec at i = 1..40, ap11 = the
 *   same at i = 0, 4, .., 40 (NaN for a class without ground truth); nthr (C-1,K) int32.
 * finalize_kitti_groups: the same per (group, class, combination) over the member records (record_groups as
 *   dpft_dataset_ap_finalize_groups_f64 takes it) with the group's own ground truth group_npos (G,C-1, device: the npos
 *   finalize_groups wrote) and its own thresholds; every output gains a leading G: the bits of an ungrouped run over the
 *   group's frames.
 * ---------------------------------------------------------------------------------------- */
int dpft_dataset_ap_update_kitti_f32(const float* cls, const float* center, const float* size, const float* angle,
                                     const float* gt_box, const int32_t* gt_id, const int32_t* counts,
                                     const double* iou_thrs, const int32_t* kinds, int32_t K, const float* roi6,
                                     float min_score, void* scratch, void* records, int64_t capacity, int64_t reserved,
                                     int64_t* counters, int32_t first_frame, int32_t B, int32_t N, int32_t Mmax,
                                     int32_t C, const void* const* desc_ptrs, const int32_t* desc_types,
                                     const double* desc_host, const int32_t* axis_cols, const int32_t* axis_counts,
                                     const int32_t* axis_values, int32_t n_axes, void* frames, int64_t frame_capacity,
                                     int64_t frames_before, void* tp_errors, int32_t ref_k, int32_t fold_pi,
                                     dpft_stream_t stream);
int dpft_dataset_ap_finalize_kitti_f64(const void* records_sorted, int64_t n_records, const int64_t* class_start,
                                       const int64_t* counters, int32_t C, int32_t K, double* ap40, double* ap11,
                                       double* prec, double* rec, double* thresholds, double* tp, double* fp,
                                       int32_t* nthr, dpft_stream_t stream);
/* HOST only (no launch): the ranks, among the n1 pass-1 TP scores in descending order, that finalize_kitti picks as
 * thresholds for npos ground-truth boxes (0 <= n1 <= npos, npos >= 1) into ranks (HOST, room for 41); returns their
 * number, 0..41, or a negative error code.  The function the kernel runs (csrc/ap_kitti.h), for tests. */
int dpft_dataset_ap_kitti_ranks(int64_t n1, int64_t npos, int64_t* ranks);
int dpft_dataset_ap_finalize_kitti_groups_f64(const void* records_sorted, const uint32_t* record_groups,
                                              int64_t n_records, const int64_t* class_start, const double* group_npos,
                                              int32_t G, int32_t C, int32_t K, double* ap40, double* ap11, double* prec,
                                              double* rec, double* thresholds, double* tp, double* fp, int32_t* nthr,
                                              dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Rotated-box NMS between the model and its consumers (dpft_amd/evaluation/nms.py states the definition; the reference
 * has no such step).  Three launches on `stream`, no read-back, no floating-point atomics: the same input gives the
 * same bits.  Per sample: candidates = queries with argmax class c != 0 (first maximum, NaN = maximum) and a non-NaN
 * score s = cls[n, c]; s >= min_score in fp32 (-INFINITY = no filter); order (score desc, query asc), -0 as +0; a
 * candidate is suppressed by the first earlier KEPT candidate (of its class unless class_agnostic) whose fp64 IoU
 * (kind 0 bev, 1 3d; the geometry of dpft_dataset_ap_update_f32) is strictly greater than `iou` (inside (0, 1)); kept
 * candidates beyond the first max_det (>= 1; INT32_MAX = no limit) are dropped.
 * status (B,N) int32: -1 kept, -2 no candidate (untouched), -3 below min_score, -4 beyond max_det, otherwise the query
 * index of the suppressor.  order (B,N): kept queries in score order, padded with -1.  counts (B).  cls_out (B,N,C):
 * the bits of cls, except [n, 0] = the row's winning score in every row of status >= 0, -3 or -4 (index 0 becomes the
 * first maximum: the query reads as background downstream).  cls_out must not alias cls.
 * `iou` points to ONE double on the HOST (the convention of iou_thrs above).
 * scratch: dpft_nms_scratch_bytes(B, N) bytes, 16-byte aligned.  N <= 1024, 2 <= C <= 16; B == 0 or N == 0 do nothing.
 * ---------------------------------------------------------------------------------------- */
int64_t dpft_nms_scratch_bytes(int32_t B, int32_t N);      /* -1 + dpft_last_error() when out of range */
int dpft_nms_f32(const float* cls, const float* center, const float* size, const float* angle, const double* iou,
                 int32_t kind, int32_t class_agnostic, float min_score, int32_t max_det, void* scratch,
                 int32_t* status, int32_t* order, int32_t* counts, float* cls_out, int32_t B, int32_t N, int32_t C,
                 dpft_stream_t stream);
/* The scratch after dpft_nms_f32, a contract for dpft_tta_vote_f32 (csrc/nms_layout.h spells the offsets): with
 * W = ceil(N / 64), in this order and unpadded, mask (B,W,W,64) uint64, then in SORTED order per sample (score desc,
 * query asc; only the first ndet[b] entries of sample b are written) box (B,N,8) float = center, size, angle,
 * label (B,N) int32, sorted (B,N) int32 = query index, score (B,N) float, and ndet (B) int32. */

/* ------------------------------------------------------------------------------------------
 * Test-time augmentation: the fusion of T views' outputs (optional, "evaluate.tta"; dpft_amd/evaluation/tta.py states
 * the definition, tests/tta_ref.py restates it).  T = 2 .. DPFT_TTA_MAX_VIEWS views of N queries, view 0 the identity;
 * M = T N <= 1024 candidates, id m = t N + n; 2 <= C <= 16.  Per batch gather, dpft_nms_f32 on the union, vote: five
 * launches on `stream`, no read-back, no atomics -- the same input gives the same bits.
 * dpft_tta_gather_f32: the views' tensors (B,N,C) (B,N,3) (B,N,3) (B,N,2) -> the union tensors (B,M,.); a view with
 *   flip != 0 has the sign bit of center[1] and angle[0] flipped.  The pointers travel by value in the kernel arguments.
 * clustering: dpft_nms_f32(union..., iou, kind, 0, min_score, INT32_MAX, scratch, status, order, counts, cls_out, B, M, C)
 *   with scratch of dpft_tta_scratch_bytes(B, N, T) (= dpft_nms_scratch_bytes(B, M)) bytes.
 * dpft_tta_vote_f32: reads the union, `status` and the sorted arrays of `scratch`.  A kept candidate heads a cluster, its
 *   members are the candidates whose status names it, visited in sorted order, head first.  w_i = (double) s_i if
 *   0 < s_i < inf else 0.  A head with n >= 2 members and sum w > 0: center and size = sum w_i x_i / sum w_i; angle =
 *   sum' w_i u_i / sum' w_i, u_i = (sin, cos) / sqrt(sin^2 + cos^2), sum' leaving out members with u_i . u_head < 0
 *   (sum' w = 0: the head's angle); all in fp64, sequential, rounded to fp32 once.  Otherwise the head's 8 floats.
 *   score 0 (mean): sum s_i / max(n, T) in fp64, rounded once; 1 (max): the head's score.  A head's row of cls_out
 *   (dpft_nms_f32's, rewritten in place) becomes zeros but [c] = the fused score; every other row of cls_out stays
 *   dpft_nms_f32's; center_out / size_out / angle_out (B,M,.) hold the union's bits in every row that is no head.
 *   members (B,M) int32: n in a head's row, 0 elsewhere.
 * ---------------------------------------------------------------------------------------- */
#define DPFT_TTA_MAX_VIEWS 4
typedef struct dpft_tta_views {
    const float* cls[DPFT_TTA_MAX_VIEWS];
    const float* center[DPFT_TTA_MAX_VIEWS];
    const float* size[DPFT_TTA_MAX_VIEWS];
    const float* angle[DPFT_TTA_MAX_VIEWS];
    int32_t flip[DPFT_TTA_MAX_VIEWS];
} dpft_tta_views;
int64_t dpft_tta_scratch_bytes(int32_t B, int32_t N, int32_t T);      /* -1 + dpft_last_error() when out of range */
int dpft_tta_gather_f32(const dpft_tta_views* views, int32_t T, float* cls, float* center, float* size, float* angle,
                        int32_t B, int32_t N, int32_t C, dpft_stream_t stream);
int dpft_tta_vote_f32(const float* center, const float* size, const float* angle, const int32_t* status,
                      const void* scratch, int32_t score, int32_t T, float* cls_out, float* center_out, float* size_out,
                      float* angle_out, int32_t* members, int32_t B, int32_t N, int32_t C, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K-Radar export selection: KRadarExporter._construct_objects
 * (src/dprt/evaluation/exporters/kradar.py:231-294) for all B samples and T <= 8 confidence thresholds at once.
 * cls (B,N,C) raw scores, center (B,N,3), size (B,N,3), angle (B,N,2)=[sin,cos]; conf_thrs is a HOST array of T
 * floats.  An object survives threshold t iff  argmax(cls)-1 >= 0  &  max(cls) >= thr_t  &  0<x<72, -6.4<y<6.4,
 * -2<z<6, -50<yaw<50 (:268-277).  rows (B,T,N,8) receives the survivors in candidate order as
 * [category, h, w, l, y, z, x, theta] (the non-constant columns of :283-292), counts (B,T) their number;
 * mask (B,N) (optional, may be NULL) bit t = survived threshold t.  One block per sample.
 * ---------------------------------------------------------------------------------------- */
int dpft_export_select_f32(const float* cls, const float* center, const float* size, const float* angle,
                           const float* conf_thrs, int32_t T, float* rows, int32_t* counts, uint8_t* mask,
                           int32_t B, int32_t N, int32_t C, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Radar tesseract -> RA / EA feature maps: KRadarProcessor.get_radar_data,
 * src/dprt/datasets/kradar/processor.py:588-633.  tesseract (D,R,E,A) linear power; doppler_raster (D);
 * ra (R,A,6), ea (E,A,6) = (rcs max, rcs median, rcs var, doppler peak, doppler centre, doppler var); the EA map
 * folds the range bins [r_lo, r_hi) (reference: 4, 252).  scratch: dpft_radar_projection_scratch_floats(D,R,E,A);
 * D <= 64, folded axes <= 256 elements.
 * ---------------------------------------------------------------------------------------- */
int64_t dpft_radar_projection_scratch_floats(int32_t D, int32_t R, int32_t E, int32_t A);
int dpft_radar_projection_f32(const float* tesseract, const float* doppler_raster, float* ra, float* ea,
                              float* scratch, int32_t D, int32_t R, int32_t E, int32_t A, int32_t r_lo,
                              int32_t r_hi, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused multi-tensor AdamW (torch.optim.AdamW semantics: decoupled decay, bias correction, no amsgrad),
 * the optimizer the reference builds at src/dprt/training/trainer.py:233 / optimizer.py:6-7.
 * chunks: device array of {float* p; const float* g; float* m; float* v; int32 n; int32 tensor}
 * (4 pointers + 2 int32 = 40 bytes each); active: device int32 per tensor (0 = skip: gradient is None) or NULL.
 * skipped (or NULL): device int32 per tensor, the number of steps the tensor sat out; its bias corrections use
 * step - skipped[t] (the per-parameter state["step"] of torch.optim.AdamW).  A row with m == NULL is the tensor's
 * "marker row": it carries no elements and advances skipped[t] when the tensor is inactive (one such row per tensor).
 * gate (round 5, or NULL): device float, the step's loss -- the reference steps only `if loss > 0` (training/trainer.py:131);
 * with a gate that is not positive every tensor sits the launch out as if it had no gradient, so the host need not read the
 * loss back before it launches the backward and the optimizer.
 * ---------------------------------------------------------------------------------------- */
int dpft_adamw_f32(const void* chunks, int32_t n_chunks, const int32_t* active, int32_t* skipped, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int32_t step, const float* gate, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Gradient clipping by global L2 norm on the device (torch.nn.utils.clip_grad_norm_, norm_type 2,
 * error_if_nonfinite=False), an extension: the reference does not clip.  Three launches, no host read-back:
 *
 * dpft_grad_sqnorm_f32: partials[r] = sum of g^2 over chunk row r of the table dpft_adamw_f32 reads (same `chunks`, same
 * `active`), one workgroup per row.  Every element is widened to double before it is squared (an fp32 square is exact in
 * fp64: no overflow at 3e19, no flush at 1e-30) and summed in double in a fixed order.  A marker row and a row of an
 * inactive tensor write 0.0.  No atomics: the partials are the same bits from run to run.  Several tables (parameter
 * groups) write disjoint ranges of one `partials` buffer.
 *
 * dpft_grad_clip_coef_f32: ONE workgroup sums partials[0 .. n_partials) in a fixed order to S and writes the 16-byte clip
 * record {float norm; float coef; int32 nonfinite; int32 nonfinite_total}: norm = (float)sqrt(S) (the norm BEFORE
 * clipping, as torch returns it), coef = (float)min(1, max_norm / (sqrt(S) + 1e-6)) evaluated in fp64 and rounded once.
 * max_norm must be finite and positive; it crosses the boundary as a float, so the coefficient is that of the fp32-rounded
 * max_norm (0.1 -> 0.100000001490116: 1.5e-8 relative, a fraction of the coefficient's own fp32 rounding).  S not finite: nonfinite = 1 (else 0) and, by nonfinite_mode,
 *   0 "propagate" (torch's behaviour): coef is what the formula gives -- NaN for a NaN norm, 0 for an infinite one;
 *   1 "skip": coef = -1, which tells dpft_adamw_clip_f32 to sit the step out, and nonfinite_total += 1.
 * nonfinite_total is only ever incremented: the caller zeroes the record once, when it allocates it.
 *
 * dpft_adamw_clip_f32: dpft_adamw_f32 with every gradient element replaced by g * record->coef in registers.  Nothing
 * is written back to the gradients: they stay unclipped in memory.  coef == 1 gives the results of dpft_adamw_f32 to the
 * bit.  coef < 0 closes the launch exactly as a gate that is not positive does: no parameter or moment moves and
 * skipped[t] advances for every tensor.
 * ---------------------------------------------------------------------------------------- */
int dpft_grad_sqnorm_f32(const void* chunks, int32_t n_chunks, const int32_t* active, double* partials,
                         dpft_stream_t stream);
int dpft_grad_clip_coef_f32(const double* partials, int32_t n_partials, float max_norm, int32_t nonfinite_mode,
                            void* record, dpft_stream_t stream);
int dpft_adamw_clip_f32(const void* chunks, int32_t n_chunks, const int32_t* active, int32_t* skipped, float lr,
                        float beta1, float beta2, float eps, float weight_decay, int32_t step, const float* gate,
                        const void* record, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Exponential moving average (EMA) of the weights inside the AdamW launch, an extension: the reference keeps none.
 *
 * dpft_adamw_ema_f32: dpft_adamw_clip_f32 (record != NULL) or dpft_adamw_f32 (record == NULL: unclipped) that also keeps
 * ema += (p_new - ema) * w for every element it updates -- ema.lerp_(p, 1 - d), the rule of
 * torch.optim.swa_utils.get_ema_multi_avg_fn -- while the new p is still in registers: one more read-modify-write per
 * element, no extra launch.  Buffer layout: `ema` is a third flat fp32 buffer per table with exactly the offsets of the
 * moments; the chunk rows stay 40 bytes, the launch gets the table's moment base `m_base` and `ema_base`, and a row's
 * slice is ema_base + (row.m - m_base).  It has the alignment of m and is accessed the way m is.
 * w = (float)(1 - d_eff), d_eff in double: d_eff = ema_decay (in [0, 1), crossing the boundary as a float), or with
 * ema_warmup == 1 min(ema_decay, (1 + own) / (10 + own)), own = step - skipped[t] the tensor's own AdamW step count (step
 * with skipped == NULL).  Sitting out: a row that dpft_adamw_f32 / dpft_adamw_clip_f32 would not update -- gate not
 * positive, record->coef < 0, inactive tensor, marker row -- leaves ema untouched: the average of a tensor advances
 * exactly when the tensor is updated.  p, m, v and skipped come out bit-equal to the launch without the average.
 *
 * dpft_swap_f32: exchanges pairs of disjoint fp32 ranges in place (the live weights and their EMA, for validation and
 * checkpoints; raw pointers, so a parameter's physical element order does not matter and no scratch copy is needed).
 * rows: device array of {float* a; float* b; int32 n; int32 pad} (24 bytes each), one workgroup of 256 per row; 16-byte
 * accesses where both pointers are 16-byte aligned and four elements remain, scalar accesses otherwise.
 * ---------------------------------------------------------------------------------------- */
int dpft_adamw_ema_f32(const void* chunks, int32_t n_chunks, const int32_t* active, int32_t* skipped, float lr,
                       float beta1, float beta2, float eps, float weight_decay, int32_t step, const float* gate,
                       const void* record, const float* m_base, float* ema_base, float ema_decay, int32_t ema_warmup,
                       dpft_stream_t stream);
int dpft_swap_f32(const void* rows, int32_t n_rows, dpft_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Measurement aid (bench.py `roofline`): while started, every dpft_conv2d_nhwc_* call is bracketed
 * by HIP events on its launch stream.  Not thread-safe; do not use inside a graph capture.
 * ---------------------------------------------------------------------------------------- */
int dpft_profile_start(void);
/* on != 0: the ResNet plans keep weight gradients / weight transposes on the main stream (no side stream) WITHOUT event
 * brackets, so that an external tracer (rocprofv3 --kernel-trace) sees every conv kernel running alone: the same
 * serialized step bench.py brackets, reproducible from a profile.  Off by default. */
int dpft_profile_serialize(int32_t on);
int32_t dpft_profile_stop(void);                 /* -> number of recorded launches */
float dpft_profile_overhead_ms(void);            /* elapsed time of an empty event bracket, calibrated by
                                                    dpft_profile_start and already subtracted by dpft_profile_get */
/* kind 0 fwd / 1 dgrad / 2 wgrad; flops = algorithmic 2*M*K*kh*kw*C; ms = event-timed duration;
 * shape7 = B,H,W,C,K,k,stride.  The stream must have been synchronised. */
int dpft_profile_get(int32_t i, int32_t* kind, double* flops, float* ms, int32_t* shape7);
/* the pipe record i was launched on, written by the dispatch code (not derived from the shape): 0 fp32 MFMA
 * (v_mfma_f32_32x32x2_f32), 1 three-term bf16 split (six v_mfma_f32_32x32x16_bf16 per fp32 product, conv_x3.hip),
 * 2 bf16 operands on the bf16 MFMA (mixed precision), 3 no matrix core (thin-channel / 16-channel / generic kernels).
 * bench.py prices every conv against ITS pipe's peak (roofline.frac_blended). */
int dpft_profile_get_family(int32_t i, int32_t* family);

#ifdef __cplusplus
}
#endif
#endif /* DPFT_HIP_H */
