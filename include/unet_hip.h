/*
 * libunet_hip.so -- C-ABI of the MI355X-native U-Net anomaly-segmentation hot path.
 *
 * The reference (ukeSJTU/tiaozhanbei-unet) has no FFI: its hot path is reached through
 * Python objects (src/model.py, src/train_utils.py) and the arithmetic lives in ATen.
 * This header is the boundary BELOW those Python objects: every entry point names the
 * reference call site (file:line under /root/reference) whose arithmetic it replaces.
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers + sizes; no torch types.  All device tensors are dense NHWC
 *     ("channels last": [N][H][W][C], C fastest) in the compute dtype (UNET_F32 or
 *     UNET_BF16) unless a parameter says otherwise; parameters/gradients of the model
 *     are fp32 in PyTorch's own layouts (OIHW etc.).
 *   - the caller owns every buffer (inputs, outputs, workspace); the library keeps no
 *     device state, never allocates or frees device memory and never synchronises:
 *     all work is enqueued on `stream` (a hipStream_t passed as void*).
 *   - return value: UNET_OK (0) or a negative unet_status; unet_last_error() gives the
 *     thread-local text of the last failure.  No C++ exception crosses the ABI.
 *     A dtype other than UNET_F32 / UNET_BF16 is UNET_ERR_BAD_ARG, reported before anything is launched.
 *   - `unet_view` places an NHWC tensor inside a larger logical frame: it is how the
 *     skip-concat (`torch.cat([x2, x1], 1)`, src/model.py:65) and the centre pad
 *     (`F.pad`, src/model.py:57-61) are expressed without ever materialising them.
 */
#ifndef UNET_HIP_H_
#define UNET_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UNET_ABI_VERSION 1

enum unet_dtype { UNET_F32 = 0, UNET_BF16 = 1 };

enum unet_status {
  UNET_OK = 0,
  UNET_ERR_BAD_ARG = -1,      /* null pointer / negative size / inconsistent description */
  UNET_ERR_UNSUPPORTED = -2,  /* shape outside what the kernels cover (see each function)  */
  UNET_ERR_WORKSPACE = -3,    /* workspace too small                                        */
  UNET_ERR_LAUNCH = -4        /* HIP reported a launch error (text in unet_last_error)      */
};

/* An NHWC tensor [n][h][w][c] whose pixel (0,0) sits at (off_y, off_x) of a logical frame.
 * Reads outside the tensor give 0; writes outside are dropped. */
typedef struct unet_view {
  void* ptr;
  int32_t c;
  int32_t h, w;
  int32_t off_y, off_x;
} unet_view;

int32_t unet_abi_version(void);
const char* unet_last_error(void);

/* Data parallelism (no reference counterpart): CUs the persistent one-block-per-CU kernels leave free for
 * the RCCL all-reduce kernels that overlap the backward pass.  The statically partitioned conv / weight-gradient /
 * transposed-conv launchers size their grids by unet_get_cu_budget() = (multiprocessor count - reserved) rounded down
 * to a multiple of 8 XCDs.  Default 0 (or UNET_RESERVED_CUS); ddp.py sets it when the world size is > 1. */
int32_t unet_set_reserved_cus(int32_t n);
int32_t unet_get_cu_budget(void);
/* Diagnostic (tools/cu_share_probe.py): `blocks` workgroups holding `lds_bytes` of LDS spin for `microseconds` on `stream`
 * -- a stand-in for resident collective kernels, to measure what CU sharing costs the persistent kernels. */
int32_t unet_debug_spin(int32_t blocks, int32_t lds_bytes, int32_t microseconds, void* stream);

/* ---- per-kernel-class timing (used by bench.py for the roofline object) -------------- */
enum unet_kclass {
  UNET_K_CONV_FWD = 0, UNET_K_CONV_DGRAD, UNET_K_CONV_WGRAD, UNET_K_CONVT_FWD, UNET_K_CONVT_DGRAD,
  UNET_K_CONVT_WGRAD, UNET_K_BN, UNET_K_POOL, UNET_K_HEAD, UNET_K_LOSS, UNET_K_PACK, UNET_K_OTHER,
  UNET_K_COUNT
};
/* When enabled, every launch of a timed class is bracketed by hipEvents on its own stream. */
int32_t unet_prof_enable(int32_t on);
/* Synchronises the recorded events; fills ms[UNET_K_COUNT], launches[UNET_K_COUNT],
 * flops[UNET_K_COUNT] (algorithmic FLOPs summed over the launches) and clears the log. */
int32_t unet_prof_collect(double* ms, int64_t* launches, double* flops);
/* Per-KERNEL breakdown of the brackets consumed by the last unet_prof_collect(): entry `index` (0, 1, ... until
 * UNET_ERR_BAD_ARG) -> kernel name (static string), summed event time, launches, algorithmic FLOPs. */
int32_t unet_prof_kernel_stats(int32_t index, const char** name, double* ms, int64_t* launches, double* flops);
/* Algorithmic bytes (inputs + weights + outputs, each once) summed over the launches of entry `index` of the same
 * breakdown; 0 for kernels whose launcher does not state them (the figure roofline.traffic is held against). */
int32_t unet_prof_kernel_bytes(int32_t index, double* bytes);

/* ---- layout ------------------------------------------------------------------------- */
/* NCHW fp32 -> NHWC compute dtype with the channel dim zero-padded to c_pad
 * (the `.to(device)` batch of src/train_utils.py:118 entering src/model.py:190). */
int32_t unet_nchw_to_nhwc(const float* src, void* dst, int32_t n, int32_t c, int32_t h, int32_t w,
                          int32_t c_pad, int32_t dtype, void* stream);
/* NHWC compute dtype (row stride c_pad) -> NCHW fp32, first c channels. */
int32_t unet_nhwc_to_nchw(const void* src, float* dst, int32_t n, int32_t c, int32_t h, int32_t w,
                          int32_t c_pad, int32_t dtype, void* stream);

/* ---- weight packing: fp32 parameters -> GEMM operand layouts in the compute dtype ------ */
enum unet_pack_mode {
  UNET_PACK_CONV_FWD = 0,   /* Conv2d w[co][ci][3][3]   -> [9][co_rows][ci_k]            */
  UNET_PACK_CONV_DGRAD = 1, /* same weight              -> [9 flipped][ci_rows][co_k]    */
  UNET_PACK_CONVT_FWD = 2,  /* ConvTranspose2d w[ci][co][2][2] -> [4][co_rows][ci_k]     */
  UNET_PACK_CONVT_DGRAD = 3 /* same weight              -> [ci_rows][4*co_k]             */
};
/* rows / k are the padded GEMM dims (zero filled); c_out, c_in are the parameter's dims. */
int32_t unet_pack_weight(const float* w, void* out, int32_t c_out, int32_t c_in, int32_t rows,
                         int32_t k, int32_t mode, int32_t dtype, void* stream);

/* All of a model's weights in ONE launch (after each optimiser step): `descs` is a DEVICE array of n
 * descriptors (the fields of unet_pack_weight; dtype is per call).  `reserved` of a 3x3 conv descriptor is the segment
 * map of its input channels (unet_pack_weight_seg's `split`); 0 = the contiguous layout. */
typedef struct unet_pack_desc {
  const float* w;
  void* out;
  int32_t c_out, c_in, rows, k, mode, reserved;
} unet_pack_desc;
int32_t unet_pack_weights_batched(const unet_pack_desc* descs, int32_t n, int32_t dtype, void* stream);

/* ---- channel widths that are not multiples of 64 (widths.hip) ----------------------------------------------------
 * DoubleConv / Down / Up / OutConv with any widths (src/model.py:9-75): a layer of c channels runs as the layer of
 * cp = pad64(c) channels with zero weight rows / columns and zero BatchNorm gamma / beta in the pad lanes, so every
 * activation and gradient keeps exactly 0 in its pad lanes through the existing kernels.
 *
 * The 3x3 conv weight of an Up block whose skip (source 0) has split = c0 % 64 != 0 channels: packed input column q
 * holds parameter column q for q < c0, zero for c0 <= q < pad64(c0) and parameter column q - pad64(c0) + c0 after that
 * (source 1 starts at pad64(c0)).  mode: UNET_PACK_CONV_FWD or UNET_PACK_CONV_DGRAD; split = 0 is unet_pack_weight. */
int32_t unet_pack_weight_seg(const float* w, void* out, int32_t c_out, int32_t c_in, int32_t rows, int32_t k,
                             int32_t mode, int32_t split, int32_t dtype, void* stream);
/* unet_pack_conv_weight_folded through the same segment map. */
int32_t unet_pack_conv_weight_folded_seg(const float* w, const float* scale, void* out, int32_t c_out, int32_t c_in,
                                         int32_t rows, int32_t k, int32_t split, int32_t dtype, void* stream);

/* fp32 tensor [rows][cols][inner] (the parameter's shape: a BatchNorm vector is [1][c][1], a conv weight
 * [co][ci][9], a transposed-conv weight [ci][co][4], a head weight [co][ci][1]) <-> its padded form
 * [prows][pcols][inner], columns through the segment map `split` (0 = contiguous).  UNET_REMAP_PAD writes the whole
 * padded tensor (zeros outside the logical one); UNET_REMAP_UNPAD writes the logical tensor from the padded one.
 * descs: HOST array of n descriptors, UNET_REMAP_MAX per launch. */
enum unet_remap_op { UNET_REMAP_PAD = 0, UNET_REMAP_UNPAD = 1 };
#define UNET_REMAP_MAX 8
typedef struct unet_remap_desc {
  const float* src;
  float* dst;
  int32_t rows, cols, inner;
  int32_t prows, pcols;
  int32_t split, op, reserved;
} unet_remap_desc;
int32_t unet_remap_batched(const unet_remap_desc* descs, int32_t n, void* stream);

/* The gradient w.r.t. a narrow block's logical-shape output -> dense NHWC [n][h][w][c_pad] in `dtype`, 0 in the pad
 * lanes.  src: [n][c][h][w] of src_dtype (UNET_F32 / UNET_BF16) with element strides strides[4] (HOST, NCHW order). */
int32_t unet_widen_channels(const void* src, int32_t src_dtype, const int64_t* strides, int32_t n, int32_t c, int32_t h,
                            int32_t w, void* dst, int32_t c_pad, int32_t dtype, void* stream);

/* ---- 3x3 convolution, pad 1, stride 1, no bias (nn.Conv2d at src/model.py:14,17) ------ */
/* y = conv(concat(src[0], src[1])) as an implicit GEMM on MFMA.  Output channels below
 * dst_split go to dst[0], the rest to dst[1] (dst[1].ptr may be NULL when dst_split == c_out).
 * The same entry computes the data gradient when given UNET_PACK_CONV_DGRAD weights:
 * dX = conv(dY, flipped W^T).  `accumulate` is a bit mask: bit 0 -> dst[0] += result, bit 1 -> dst[1] += result
 * (gradient fan-in of the skip connections: the three consumers of a skip tensor add into one buffer).
 * Requires: channel counts of each src multiples of 64 (or a single src of 8/16 for the
 * image layer), c_out multiple of 64.  Narrower layers (any width c) run as the pad64(c) layer with zero pad lanes
 * (widths section below), doing pad64(c)/c times the useful MFMA work: a 32-wide layer runs a 64-wide GEMM. */
int32_t unet_conv3x3(int32_t dtype, int32_t n, int32_t h, int32_t w, const unet_view src[2],
                     const void* w_packed, int32_t c_out, const unet_view dst[2], int32_t dst_split,
                     int32_t accumulate, int32_t kclass, void* stream);

/* Inference form of conv + BatchNorm(eval) + ReLU (src/model.py:14-19 under model.eval(), src/test.py:68): BatchNorm's
 * running statistics are folded into the layer -- scale = gamma / sqrt(running_var + eps) into the packed weights
 * (unet_pack_conv_weight_folded; scale / shift from unet_bn_eval_coeffs), shift = beta - running_mean * scale as the
 * bias of the convolution's epilogue, followed by max(., 0) when relu != 0.  One kernel per layer, the activation is
 * written once (y: dense NHWC [n][h][w][c_out] in the compute dtype). */
int32_t unet_pack_conv_weight_folded(const float* w, const float* scale, void* out, int32_t c_out, int32_t c_in,
                                     int32_t rows, int32_t k, int32_t dtype, void* stream);
int32_t unet_conv3x3_bias_relu(int32_t dtype, int32_t n, int32_t h, int32_t w, const unet_view src[2],
                               const void* w_packed, int32_t c_out, void* y, const float* bias, int32_t relu,
                               void* stream);

/* The FIRST convolution of the network (inc.double_conv.0: nn.Conv2d(n_channels, 64, 3, padding=1), src/model.py:14
 * reached from UNet.forward :98 / AnomalyUNet.forward :190), bf16 mode, straight from the caller's fp32 NCHW image
 * and fp32 OIHW weight: with 9*c_in <= 32 the whole reduction is one 32-deep MFMA step, so the image is never padded
 * to 64 channels.  y: bf16 NHWC [n][h][w][64].  partial (may be NULL: no statistics) receives *n_parts ordered
 * BatchNorm partials [part][2][64] for unet_bn_finalize_partials (capacity: unet_conv3x3_stats_max_parts).
 * unet_conv3x3_first_supported() tells whether a layer qualifies (c_out == 64, 9*c_in <= 32, w % 16 == 0). */
int32_t unet_conv3x3_first_supported(int32_t c_in, int32_t c_out, int32_t h, int32_t w);
int32_t unet_conv3x3_first_stats(int32_t n, int32_t h, int32_t w, const float* x_nchw, int32_t c_in,
                                 const float* weight_oihw, void* y, float* partial, int32_t* n_parts, void* stream);
/* dW[64][c_in][3][3] (fp32) = sum over pixels of dY (bf16 NHWC) x the shifted image; ordered reductions. */
size_t unet_conv3x3_first_wgrad_workspace(int32_t n, int32_t h, int32_t w);
int32_t unet_conv3x3_first_wgrad(int32_t n, int32_t h, int32_t w, const float* x_nchw, int32_t c_in, const void* dy,
                                 float* dw, void* workspace, size_t workspace_bytes, void* stream);
/* The same weight gradient with the BatchNorm-backward apply of the layer (src/model.py:15, autograd) folded in: the
 * image layer's dy has no other consumer (no data gradient towards the image), so instead of a standalone pass
 * dy = A*dz + B*y + K the kernel streams the ReLU-masked gradient dz and the raw conv output y (both bf16 NHWC
 * [n][h][w][64]) and forms dy -- rounded to bf16 as the pass stored it: bit-identical dW -- on its operand.
 * coefs: DEVICE [3][64] = A, B, K, as unet_bn_bwd_premasked leaves them in its workspace when called with dy = NULL. */
int32_t unet_conv3x3_first_wgrad_bn(int32_t n, int32_t h, int32_t w, const float* x_nchw, int32_t c_in, const void* dz,
                                    const void* y, const float* coefs, float* dw, void* workspace,
                                    size_t workspace_bytes, void* stream);

/* The forward convolution of DoubleConv fused with the BatchNorm batch statistics (src/model.py:14-15,
 * 17-18): y = conv(concat(src)) AND per-channel partial sums (sum, sum of squares of the stored y) written
 * by the conv epilogue through wavefront reductions -- or, for kernel variants without that epilogue, by one
 * extra streaming pass.  partial: fp32 [parts][2][c_out], capacity unet_conv3x3_stats_max_parts() parts;
 * *n_parts receives the number written.  Feed them to unet_bn_finalize_partials(). */
size_t unet_conv3x3_stats_max_parts(int32_t n, int32_t h, int32_t w);
int32_t unet_conv3x3_stats(int32_t dtype, int32_t n, int32_t h, int32_t w, const unet_view src[2],
                           const void* w_packed, int32_t c_out, void* y, float* partial, int32_t* n_parts,
                           void* stream);

/* Data gradient of the SECOND convolution of DoubleConv (src/model.py:17) fused with the backward of the ReLU and
 * the reduction half of the BatchNorm2d backward of the FIRST one (src/model.py:15-16), whose activation is this
 * convolution's only input: dz = conv(dy, flipped W^T) * [fma(y_prev, bn_scale, bn_shift) > 0] (dense NHWC
 * [n][h][w][c_dx], compute dtype) and partial[*n_parts][2][c_dx] = per-channel (sum dz, sum dz * (y_prev - bn_mean))
 * of the stored dz, written by the kernel's epilogue -- feed both to unet_bn_bwd_premasked.  The (y, da) reduction pass
 * of unet_bn_relu_bwd does not exist on this route.  w_packed = UNET_PACK_CONV_DGRAD [9][c_dx][c_dy]; partial capacity:
 * unet_conv3x3_stats_max_parts(n, h, w) parts.  unet_conv3x3_dgrad_bnrelu_supported() says whether a shape is covered
 * (bf16, 16-aligned frames, c_dy >= 128); otherwise use unet_conv3x3 + unet_bn_relu_bwd. */
int32_t unet_conv3x3_dgrad_bnrelu_supported(int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c_dy, int32_t c_dx);
int32_t unet_conv3x3_dgrad_bnrelu(int32_t dtype, int32_t n, int32_t h, int32_t w, const void* dy, int32_t c_dy,
                                  const void* w_packed, int32_t c_dx, const void* y_prev, const float* bn_scale,
                                  const float* bn_shift, const float* bn_mean, void* dz, float* partial,
                                  int32_t* n_parts, void* stream);

/* dW[co][ci][3][3] (fp32, OIHW) = sum over pixels of dY (x) shifted X; split-K over pixel
 * tiles with fp32 partial slabs in `workspace`, reduced in a fixed order (deterministic).
 * (autograd of nn.Conv2d, reached from total_loss.backward() at src/train_utils.py:132) */
size_t unet_conv3x3_wgrad_workspace(int32_t n, int32_t h, int32_t w, int32_t c_in, int32_t c_out);
int32_t unet_conv3x3_wgrad(int32_t dtype, int32_t n, int32_t h, int32_t w, const unet_view src[2],
                           const void* dy, int32_t c_out, float* dw, int32_t c_in_param,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---- 2x2 stride-2 transposed convolution with bias (nn.ConvTranspose2d, src/model.py:51) */
/* y[n][2i+k][2j+l][co] = b[co] + sum_ci x[n][i][j][ci] * w[ci][co][k][l]  (one GEMM + pixel shuffle) */
int32_t unet_convt2x2_fwd(int32_t dtype, int32_t n, int32_t h, int32_t w, const void* x, int32_t c_in,
                          const void* w_packed, const float* bias, void* y, int32_t c_out, void* stream);
/* dx from dy (dy is the [n][2h][2w][c_out] gradient); w_packed = UNET_PACK_CONVT_DGRAD. */
int32_t unet_convt2x2_dgrad(int32_t dtype, int32_t n, int32_t h, int32_t w, const void* dy,
                            int32_t c_out, const void* w_packed, void* dx, int32_t c_in, void* stream);

/* The same data gradient when the transposed convolution's input is the activation of a conv-BatchNorm-ReLU layer with
 * no other consumer (the DoubleConv in front of an Up block: src/model.py:14-19 -> :51, autograd of Up.forward :55):
 * the epilogue applies that layer's ReLU mask (from its raw conv output y_prev and scale/shift) and reduces the
 * BatchNorm-backward sums, as unet_conv3x3_dgrad_bnrelu does for a 3x3 consumer.  dz = masked gradient
 * [n][h][w][c_in]; partial = [unet_convt2x2_dgrad_bnrelu_max_parts()][2][c_in] floats (sum dz, sum dz*(y-mean)),
 * *n_parts rows written; finish with unet_bn_bwd_premasked. */
int32_t unet_convt2x2_dgrad_bnrelu_supported(int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c_in, int32_t c_out);
size_t unet_convt2x2_dgrad_bnrelu_max_parts(void);
int32_t unet_convt2x2_dgrad_bnrelu(int32_t dtype, int32_t n, int32_t h, int32_t w, const void* dy, int32_t c_out,
                                   const void* w_packed, const void* y_prev, const float* bn_scale, const float* bn_shift,
                                   const float* bn_mean, void* dz, int32_t c_in, float* partial, int32_t* n_parts,
                                   void* stream);
size_t unet_convt2x2_wgrad_workspace(int32_t n, int32_t h, int32_t w, int32_t c_in, int32_t c_out);
/* dw[ci][co][2][2], db[co] in fp32. */
int32_t unet_convt2x2_wgrad(int32_t dtype, int32_t n, int32_t h, int32_t w, const void* x, int32_t c_in,
                            const void* dy, int32_t c_out, float* dw, float* db, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ---- BatchNorm2d (+ ReLU) (nn.BatchNorm2d / nn.ReLU at src/model.py:15-16,18-19) -------- */
size_t unet_bn_workspace(int64_t pixels, int32_t c);
/* training statistics of y[pixels][c]: biased variance for normalisation, running stats
 * updated with `momentum` towards mean / UNBIASED variance (running_* may be NULL).
 * Outputs (fp32[c]): save_mean, save_istd, scale = gamma*istd, shift = beta - mean*scale. */
int32_t unet_bn_train_stats(int32_t dtype, const void* y, int64_t pixels, int32_t c, const float* gamma,
                            const float* beta, float* running_mean, float* running_var, float momentum,
                            float eps, float* save_mean, float* save_istd, float* scale, float* shift,
                            void* workspace, size_t workspace_bytes, void* stream);
/* same outputs as unet_bn_train_stats, from partial sums [n_parts][2][c] (ordered fp64 reduction). */
int32_t unet_bn_finalize_partials(const float* partial, int32_t n_parts, int64_t pixels, int32_t c,
                                  const float* gamma, const float* beta, float* running_mean,
                                  float* running_var, float momentum, float eps, float* save_mean,
                                  float* save_istd, float* scale, float* shift, void* stream);
/* eval: scale/shift from the running statistics. */
int32_t unet_bn_eval_coeffs(int32_t c, const float* gamma, const float* beta, const float* running_mean,
                            const float* running_var, float eps, float* scale, float* shift, void* stream);
/* eval coefficients plus the constants the FROZEN backward needs: mean = running_mean, istd = 1/sqrt(running_var+eps). */
int32_t unet_bn_eval_coeffs4(int32_t c, const float* gamma, const float* beta, const float* running_mean,
                             const float* running_var, float eps, float* mean, float* istd, float* scale,
                             float* shift, void* stream);
/* a = max(fma(y, scale, shift), 0) */
int32_t unet_bn_relu_apply(int32_t dtype, const void* y, int64_t pixels, int32_t c, const float* scale,
                           const float* shift, void* a, void* stream);
/* backward of a = relu(bn(y)) in training mode: dgamma, dbeta (fp32[c]) and
 * dy = gamma*istd*(dz - dbeta/M - yhat*dgamma/M), dz = da*[z>0]. */
int32_t unet_bn_relu_bwd(int32_t dtype, const void* da, const void* y, int64_t pixels, int32_t c,
                         const float* gamma, const float* save_mean, const float* save_istd,
                         const float* scale, const float* shift, float* dgamma, float* dbeta, void* dy,
                         void* workspace, size_t workspace_bytes, void* stream);

/* backward of a = relu(bn(y)) with FROZEN statistics (a BatchNorm2d put in eval() inside a training model -- the
 * fine-tuning pattern the reference's nn.Sequential honours, src/model.py:13-20): mean / istd are constants, so
 * dy = gamma*istd*dz; dgamma = sum dz*yhat, dbeta = sum dz as usual.  Same workspace as unet_bn_relu_bwd. */
int32_t unet_bn_relu_bwd_frozen(int32_t dtype, const void* da, const void* y, int64_t pixels, int32_t c,
                                const float* gamma, const float* mean, const float* istd, const float* scale,
                                const float* shift, float* dgamma, float* dbeta, void* dy, void* workspace,
                                size_t workspace_bytes, void* stream);
/* The same backward when the producer of the gradient has already applied the ReLU mask in its own epilogue and left
 * the two per-channel sums behind (unet_head_bnrelu_bwd, unet_conv3x3_dgrad_bnrelu): dz = da*[z>0] (compute dtype,
 * NHWC), partial = fp32 [n_parts][2][c] holding sum dz and sum dz*(y - mean).  Ordered fp64 finalize -> dgamma, dbeta,
 * then ONE pass dy = A*dz + B*y + K (dy may alias dz).  workspace: 3*c floats = A, B, K on return; dy = NULL skips the
 * pass (dz / y may then be NULL too, and dtype is not looked at): the caller's consumer applies the coefficients
 * (unet_conv3x3_first_wgrad_bn). */
int32_t unet_bn_bwd_premasked(int32_t dtype, const void* dz, const void* y, int64_t pixels, int32_t c,
                              const float* gamma, const float* save_mean, const float* save_istd,
                              const float* partial, int32_t n_parts, float* dgamma, float* dbeta, void* dy,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ---- MaxPool2d(2) (src/model.py:32): stride 2, floor; first maximum wins ties ---------- */
int32_t unet_maxpool2_fwd(int32_t dtype, const void* x, int32_t n, int32_t h, int32_t w, int32_t c,
                          void* y, void* stream);
/* accumulate != 0: dx += routed gradient (dx already holds the other consumers' gradient of x). */
int32_t unet_maxpool2_bwd(int32_t dtype, const void* x, const void* dy, int32_t n, int32_t h, int32_t w,
                          int32_t c, void* dx, int32_t accumulate, void* stream);

/* BatchNorm-apply + ReLU of an encoder level fused with the next level's MaxPool2d(2) (src/model.py:18-19 -> :32): one
 * pass over the raw conv output y writes the activation a (the skip tensor) and pooled = maxpool2(a).  The backward takes
 * the gradient other consumers already accumulated for a (da_old, NULL = none) and the pooled gradient, routes the latter
 * to the first maximum of each window, applies this layer's ReLU mask and reduces the BatchNorm-backward sums:
 * dz (may alias da_old) + partial[*n_parts][2][c] (capacity unet_bn_relu_pool_max_parts()) -> unet_bn_bwd_premasked.
 * Needs 256 % (c / 8) == 0 (bf16) or 256 % (c / 4) == 0 (fp32): unet_bn_relu_pool_supported(). */
int32_t unet_bn_relu_pool_supported(int32_t dtype, int32_t c);
int32_t unet_bn_relu_pool_fwd(int32_t dtype, const void* y, int32_t n, int32_t h, int32_t w, int32_t c,
                              const float* scale, const float* shift, void* a, void* pooled, void* stream);
size_t unet_bn_relu_pool_max_parts(void);
int32_t unet_bn_relu_pool_bwd(int32_t dtype, const void* y, const void* dpooled, const void* da_old, int32_t n, int32_t h,
                              int32_t w, int32_t c, const float* scale, const float* shift, const float* mean, void* dz,
                              float* partial, int32_t* n_parts, void* stream);
/* The same backward without ever storing dz (a streaming producer can afford to form it twice):
 *   unet_bn_relu_pool_bwd_sums   -> partial / *n_parts exactly as unet_bn_relu_pool_bwd leaves them, nothing else written;
 *   unet_bn_bwd_premasked(dz = y = dy = NULL) -> dgamma, dbeta and coefs = A, B, K in its workspace;
 *   unet_bn_relu_pool_bwd_apply  -> forms the same dz again and writes dy = A*dz + B*y + K (dy may alias da_old).
 * dy, dgamma, dbeta are bit for bit those of unet_bn_relu_pool_bwd + unet_bn_bwd_premasked(dy = dz). */
int32_t unet_bn_relu_pool_bwd_sums(int32_t dtype, const void* y, const void* dpooled, const void* da_old, int32_t n,
                                   int32_t h, int32_t w, int32_t c, const float* scale, const float* shift,
                                   const float* mean, float* partial, int32_t* n_parts, void* stream);
int32_t unet_bn_relu_pool_bwd_apply(int32_t dtype, const void* y, const void* dpooled, const void* da_old, int32_t n,
                                    int32_t h, int32_t w, int32_t c, const float* scale, const float* shift,
                                    const float* coefs, void* dy, void* stream);

/* ---- bilinear x2, align_corners=True (nn.Upsample, src/model.py:48) -------------------- */
int32_t unet_upsample_bilinear2x_fwd(int32_t dtype, const void* x, int32_t n, int32_t h, int32_t w,
                                     int32_t c, void* y, void* stream);
int32_t unet_upsample_bilinear2x_bwd(int32_t dtype, const void* dy, int32_t n, int32_t h, int32_t w,
                                     int32_t c, void* dx, void* stream);

/* ---- 1x1 head (OutConv, src/model.py:72) with optional sigmoid (src/model.py:201,208) --- */
/* x: NHWC compute dtype [pixels][c_in]; w fp32 [c_out][c_in]; out: NCHW fp32. c_out <= 8. */
int32_t unet_head_fwd(int32_t dtype, const void* x, int32_t n, int32_t h, int32_t w, int32_t c_in,
                      const float* weight, const float* bias, int32_t c_out, int32_t sigmoid, float* out,
                      void* stream);
size_t unet_head_bwd_workspace(int32_t n, int32_t h, int32_t w, int32_t c_in, int32_t c_out);
/* dout: NCHW fp32 gradient w.r.t. `out`; out: the forward result (needed when sigmoid). */
int32_t unet_head_bwd(int32_t dtype, const void* x, const float* out, const float* dout, int32_t n,
                      int32_t h, int32_t w, int32_t c_in, const float* weight, int32_t c_out,
                      int32_t sigmoid, void* dx, float* dweight, float* dbias, void* workspace,
                      size_t workspace_bytes, void* stream);

/* OutConv fed by the RAW convolution output y of the last conv-BatchNorm-ReLU layer (src/model.py:17-19 followed by
 * :72 / :107 / :200,207): a = max(fma(y, bn_scale, bn_shift), 0) is formed on load -- the activation tensor is never
 * written, its BatchNorm-apply pass does not exist.  bn_scale / bn_shift / bn_mean: outputs of
 * unet_bn_finalize_partials.  The backward recomputes a for dweight, writes dz = da*[z>0] (NHWC compute dtype) and the
 * BatchNorm-backward partial sums bn_partial[*n_parts][2][c_in] (capacity unet_head_bnrelu_max_parts() parts) for
 * unet_bn_bwd_premasked: the (y, da) reduction pass does not exist either. */
int32_t unet_head_bnrelu_fwd(int32_t dtype, const void* y, int32_t n, int32_t h, int32_t w, int32_t c_in,
                             const float* bn_scale, const float* bn_shift, const float* weight, const float* bias,
                             int32_t c_out, int32_t sigmoid, float* out, void* stream);
size_t unet_head_bnrelu_max_parts(void);
int32_t unet_head_bnrelu_bwd(int32_t dtype, const void* y, const float* bn_scale, const float* bn_shift,
                             const float* bn_mean, const float* out, const float* dout, int32_t n, int32_t h, int32_t w,
                             int32_t c_in, const float* weight, int32_t c_out, int32_t sigmoid, void* dz,
                             float* dweight, float* dbias, float* bn_partial, int32_t* n_parts, void* workspace,
                             size_t workspace_bytes, void* stream);
/* The same backward without ever storing dz (it is cheap to form again: c_out planes and the filters):
 *   unet_head_bnrelu_bwd_sums  -> dweight, dbias, bn_partial / *n_parts exactly as unet_head_bnrelu_bwd leaves them;
 *   unet_bn_bwd_premasked(dz = y = dy = NULL) -> dgamma, dbeta and coefs = A, B, K in its workspace;
 *   unet_head_bnrelu_bwd_apply -> forms the same dz again and writes dy = A*dz + B*y + K (NHWC compute dtype).
 * dy, dgamma, dbeta are bit for bit those of unet_head_bnrelu_bwd + unet_bn_bwd_premasked(dy = dz). */
int32_t unet_head_bnrelu_bwd_sums(int32_t dtype, const void* y, const float* bn_scale, const float* bn_shift,
                                  const float* bn_mean, const float* out, const float* dout, int32_t n, int32_t h,
                                  int32_t w, int32_t c_in, const float* weight, int32_t c_out, int32_t sigmoid,
                                  float* dweight, float* dbias, float* bn_partial, int32_t* n_parts, void* workspace,
                                  size_t workspace_bytes, void* stream);
int32_t unet_head_bnrelu_bwd_apply(int32_t dtype, const void* y, const float* bn_scale, const float* bn_shift,
                                   const float* out, const float* dout, int32_t n, int32_t h, int32_t w, int32_t c_in,
                                   const float* weight, int32_t c_out, int32_t sigmoid, const float* coefs, void* dy,
                                   void* stream);

/* ---- loss heads (src/train_utils.py) ----------------------------------------------------- */
size_t unet_loss_workspace(int64_t elems);
/* CombinedLoss.forward (train_utils.py:30-44): losses[0] = mean((recon-image)^2),
 * losses[1] = focal(amap, mask) (train_utils.py:23-28; BCE log clamp -100, backward
 * denominator clamp 1e-12 as ATen).  Also writes d losses[0]/d recon and d losses[1]/d amap. */
int32_t unet_loss_mse_focal(const float* recon, const float* image, int64_t n_recon, const float* amap,
                            const float* mask, int64_t n_amap, float alpha, float gamma, float* losses,
                            float* d_recon, float* d_amap, void* workspace, size_t workspace_bytes,
                            void* stream);
/* SSIMLoss (train_utils.py:67-104): 11-tap separable Gaussian (sigma 1.5), zero pad 5, NCHW fp32
 * planes.  loss[0] = 1 - mean(ssim_map); d_img1/d_img2 (may be NULL) get d loss / d img. */
size_t unet_ssim_workspace(int32_t planes, int32_t h, int32_t w);
int32_t unet_ssim_loss(const float* img1, const float* img2, int32_t planes, int32_t h, int32_t w,
                       int32_t window, float* loss, float* d_img1, float* d_img2, void* workspace,
                       size_t workspace_bytes, void* stream);

/* SSIMLoss(size_average=False) (train_utils.py:84-87): loss[i] = 1 - mean_{c,h,w} ssim_map of image i (n images of c
 * planes); d_img1 / d_img2 (may be NULL) receive d loss[i] / d img for image i.  workspace: unet_ssim_workspace(c, h, w). */
int32_t unet_ssim_loss_per_image(const float* img1, const float* img2, int32_t n, int32_t c, int32_t h, int32_t w,
                                 int32_t window, float* loss, float* d_img1, float* d_img2, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* ---- optimiser (torch.optim.Adam of get_optimizer, src/train_utils.py:266) -------------- */
/* ---- Multi-class segmentation head of the Gear/Kolektor trainers (src/metrics.py) ------------------------ */
/* CombinedSegmentationLoss.forward (src/metrics.py:300-335): loss = ce_weight * CE(class weights, ignore_index)
 * + dice_weight * dice_loss(softmax(logits)) (:233-261) + focal_weight * focal_loss (:264-282), value AND gradient.
 * logits: fp32 NCHW [n][c][hw], c <= 8; target: int64 [n][hw]; class_weights: [c] or NULL; ignore_index < 0: none.
 * input_is_prob != 0: `logits` already holds probabilities (stand-alone dice_loss(pred, target)); Dice term only.
 * loss[4] = {total, ce, dice, focal}; dlogits (same shape as logits) may be NULL.  Ordered reductions. */
size_t unet_seg_loss_workspace(int32_t n, int32_t c, int64_t hw);
int32_t unet_seg_loss(const float* logits, const int64_t* target, int32_t n, int32_t c, int64_t hw,
                      const float* class_weights, int64_t ignore_index, int32_t input_is_prob, float ce_weight,
                      float dice_weight, float focal_weight, float focal_alpha, float focal_gamma, float* loss,
                      float* dlogits, void* workspace, size_t workspace_bytes, void* stream);
/* SegmentationMetrics.update (src/metrics.py:22-45): labels[n][hw] = argmax over classes (the FIRST maximum wins
 * ties, as torch.argmax), confusion[t][p] += 1 over the pixels whose target is a class and not ignore_index.
 * labels or confusion (with target) may be NULL.  Integer atomics: exact. */
int32_t unet_seg_confusion(const float* logits, const int64_t* target, int32_t n, int32_t c, int64_t hw,
                           int64_t ignore_index, int64_t* labels, int64_t* confusion, void* stream);
/* Per-image evaluation statistics (SegmentationMetrics.update per image, visualize.py:239-257 compute_prediction_stats)
 * of fp32 NCHW logits [n][c][hw], 2 <= c <= 8, in one pass: confusion[n][c][c] (uint64 counts, rows = truth, columns =
 * prediction; the first maximum wins ties; pixels whose target is ignore_index or not a class are skipped; target NULL:
 * all zeros; confusion may be NULL), conf[n][2] (fp64) = mean and unbiased standard deviation (n - 1, torch.std) of the
 * per-pixel maximum softmax probability over all hw pixels, labels[n][hw] (uint8 argmax, may be NULL).  Ordered fp64
 * reductions through the workspace, no float atomics: bitwise reproducible.  Allocates nothing, does not synchronise.
 * The workspace query returns 0 for unsupported shapes. */
size_t unet_seg_image_stats_workspace(int32_t n, int32_t c, int64_t hw);
int32_t unet_seg_image_stats(const float* logits, const int64_t* target, int32_t n, int32_t c, int64_t hw,
                             int64_t ignore_index, uint8_t* labels, int64_t* confusion, double* conf, void* workspace,
                             size_t workspace_bytes, void* stream);

/* Pixel-level threshold epilogue of the anomaly branch (src/test.py:79-106 evaluate_results, src/train_utils.py:232-245
 * validate_epoch): for each of k <= 8 thresholds the confusion counts {tp, fp, fn, tn} of (pred > t) against
 * (truth > 0.5) over the images with select[n] != 0 (NULL: all).  counts[k][4] (int64, device) is ADDED to: zero it first.
 * pred / truth: fp32 [n_images][per_image].  Integer atomics: exact and order-independent. */
int32_t unet_threshold_confusion(const float* pred, const float* truth, const uint8_t* select, int64_t n_images,
                                 int64_t per_image, const float* thresholds, int32_t k, int64_t* counts, void* stream);

/* Pixel-level AUROC and AUPRC of the anomaly branch (src/test.py:172-178 evaluate_results -> src/utils.py:97-108
 * calculate_pixel_metrics -> :84-91 roc_auc_score, auc(precision_recall_curve) with the anomaly map as the scores),
 * without copying the maps to the host.  Two steps:
 * unet_rank_auc_append: over the images with select[n] != 0 (NULL: all) of pred / truth (fp32 [n_images][per_image]),
 * every finite score becomes an order-preserving uint32 key (-0.0 == +0.0): the keys of positive pixels (truth > 0.5,
 * as unet_threshold_confusion) are written to keys[counts[0] ...] upwards, those of negative pixels to
 * keys[capacity - 1 - counts[1] ...] downwards, in no particular order; counts[3] = {positives, negatives, non-finite
 * scores} (int64, device) is ADDED to: zero it first, and size capacity >= every selected pixel of every call that adds
 * to the same counts.  Integer atomics only; allocates nothing, does not synchronise.
 * unet_rank_auc: sorts pos_keys[n_pos] and neg_keys[n_neg] in place (LSD radix sort; 16-byte aligned arrays) and writes
 * out[2] (fp64, device) = {AUROC, AUPRC}: AUROC = sum over distinct positive keys v of pos_v (2 #neg<v + neg_v) / (2 P N)
 * (Mann-Whitney, ties counted half; the numerator in uint64, rounded once by the division), AUPRC = sum over v of
 * pos_v / P (prec(>= v) + prec(> v)) / 2, prec(> v) = 1 when nothing lies above v (sklearn's (recall 0, precision 1)
 * point).  n_pos == 0 or n_neg == 0: {0, 0}.  Non-finite scores are the caller's to handle (the reference's
 * calculate_metrics returns 0 / 0 for them).  n_pos + n_neg >= 2^31 is UNET_ERR_UNSUPPORTED (and the workspace query
 * returns 0).  Ordered reductions, no float atomics: the result depends only on the two key multisets. */
int32_t unet_rank_auc_append(const float* pred, const float* truth, const uint8_t* select, int64_t n_images,
                             int64_t per_image, uint32_t* keys, int64_t capacity, int64_t* counts, void* stream);
size_t unet_rank_auc_workspace(int64_t n_pos, int64_t n_neg);
int32_t unet_rank_auc(uint32_t* pos_keys, int64_t n_pos, uint32_t* neg_keys, int64_t n_neg, double* out,
                      void* workspace, size_t workspace_bytes, void* stream);

/* Region labelling of ground-truth masks (no reference counterpart: the per-region-overlap metric of the MVTec AD
 * evaluation needs the connected defects, which scipy.ndimage.label would find on the host).  truth: fp32 [n][h][w]; a
 * pixel is defective iff truth > 0.5 (as unet_threshold_confusion); a region is an 8-connected component of defective
 * pixels of one image.  Over the images with select[n] != 0 (NULL: all): labels[n][h][w] (int32) = 1 + the smallest
 * linear index y * w + x of the pixel's region, sizes[n][h][w] (int32) = the region's pixel count at every one of its
 * pixels; both 0 at pixels that are not defective and in images that are not selected.  counts[3] = {regions, defective
 * pixels, ok pixels} (int64, device) is ADDED to: zero it first.  Tiled union-find (LDS tiles, integer atomicMin on the
 * links across tile borders, integer atomicAdd for the sizes) in separate launches: the outputs are a function of the
 * masks alone.  Any h, w >= 1; n < 65536 and n h w <= 2^31 - 1, else UNET_ERR_UNSUPPORTED (and the workspace query
 * returns 0).  Allocates nothing, does not synchronise. */
size_t unet_label_regions_workspace(int64_t n, int64_t h, int64_t w);
int32_t unet_label_regions(const float* truth, const uint8_t* select, int64_t n, int64_t h, int64_t w, int32_t* labels,
                           int32_t* sizes, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* Class regions of uint8 label maps and their overlaps (no reference counterpart: the defect-level figures of the Gear
 * and KolektorSDD evaluation -- defects found, false alarms, parts rejected -- need the connected defects of the truth
 * and of the argmax prediction).  classes: uint8 [n][h][w]; a pixel has class c iff its value is c with
 * 1 <= c < num_classes; 0 and every value >= num_classes (255, the ignore value, among them) are background.  A class
 * region is an 8-connected component of pixels of one and the same class in one image: touching regions of different
 * classes stay apart.
 * unet_label_class_regions: region[n][h][w] (int32) = 1 + the smallest linear index y * w + x of the pixel's region (the
 * numbering of unet_label_regions), sizes[n][h][w] (int32) = the region's pixel count at every one of its pixels; both
 * 0 on background.  counts[n][num_classes] (int64, device) = regions per image and class (column 0 stays as it is) is
 * ADDED to: zero it first.  The tiled union-find of unet_label_regions with "has my class" as the union predicate.
 * unet_match_class_regions: truth / pred with the region and sizes arrays that unet_label_class_regions made of them.  A
 * predicted region is kept iff its size >= min_pixels (>= 1).  hit of a truth region = its pixels whose predicted class
 * is the region's class and whose predicted region is kept; hit of a kept predicted region = its pixels whose truth class
 * is its class.  Every truth region goes to truth_records and every kept predicted region to pred_records as one record
 * of 5 int32 {image_base + image, class, root index y * w + x, size, hit}, at the slot that an atomic add on
 * record_counts[2] = {truth, predicted} (int64, device; ADDED to: zero it first) hands out: the order is arbitrary, sort
 * by (image, root index).  capacity = records that each buffer holds; a record past it is counted and not written.
 * Integer atomics only: apart from the record order the outputs are a function of the two maps alone.
 * Both: any h, w >= 1; n < 65536, n h w <= 2^31 - 1 and 2 <= num_classes <= 255, else UNET_ERR_UNSUPPORTED before any
 * launch (and the workspace queries return 0).  Allocate nothing, do not synchronise. */
size_t unet_label_class_regions_workspace(int64_t n, int64_t h, int64_t w, int32_t num_classes);
int32_t unet_label_class_regions(const uint8_t* classes, int64_t n, int64_t h, int64_t w, int32_t num_classes,
                                 int32_t* region, int32_t* sizes, int64_t* counts, void* workspace,
                                 size_t workspace_bytes, void* stream);
size_t unet_match_class_regions_workspace(int64_t n, int64_t h, int64_t w, int32_t num_classes);
int32_t unet_match_class_regions(const uint8_t* truth, const int32_t* truth_region, const int32_t* truth_sizes,
                                 const uint8_t* pred, const int32_t* pred_region, const int32_t* pred_sizes, int64_t n,
                                 int64_t h, int64_t w, int32_t num_classes, int32_t min_pixels, int32_t image_base,
                                 int32_t* truth_records, int32_t* pred_records, int64_t capacity,
                                 int64_t* record_counts, void* workspace, size_t workspace_bytes, void* stream);

/* Groups of class regions (no reference counterpart; csrc/groups.hip, restated in numpy by tests/_groups_ref.py): which
 * regions of a prediction belong to one defect.  A U-Net breaks a thin scratch into a row of fragments a few pixels
 * apart; grouped, they are measured, filtered and paired as one.  classes, region and sizes are what
 * unet_label_class_regions takes and makes; gap in 1..32, gap_sq = gap * gap; min_pixels >= 1.  A fragment is a region
 * with size >= min_pixels; smaller regions are dropped before grouping, so they link nothing and join nothing.  Two
 * fragments of the same image and class are linked iff they hold pixels p, q with
 * (py - qy)^2 + (px - qx)^2 <= gap_sq; a group is a connected component of the link graph (linking is transitive), and
 * fragments of different classes or images are never linked.  Two distinct regions of one class are at least 2 apart,
 * so gap = 1 gives every fragment its own group.
 * group[n][h][w] (int32) = 1 + the smallest fragment root index y * w + x of the pixel's group (itself a pixel of the
 * group), group_sizes[n][h][w] (int32) = the group's pixel count at every one of its pixels; both 0 on background and
 * on dropped regions: (group, group_sizes) stands in for (region, sizes) in unet_describe_class_regions,
 * unet_measure_class_regions and unet_region_pairs.  counts[n][num_classes] (int64, device) = groups per image and
 * class (column 0 stays as it is) is ADDED to: zero it first.  Every fragment yields one record of 5 int64
 * {image_base + image, class, fragment root, group root, fragment size} at the slot that an atomic add on
 * fragment_count[1] (int64, device; ADDED to: zero it first) hands out: the order is arbitrary, sort by (image, group
 * root, fragment root).  capacity = records that the buffer holds; a record past it is counted and not written.
 * Four launches: the fragment roots link to themselves in a per-pixel link plane; a workgroup per 32 x 32 tile stages
 * the tile and its halo in LDS, and every edge pixel of a fragment (one with a 4-neighbour inside the frame that is not
 * of its region) scans the half-disc dy > 0, or dy == 0 and dx > 0, and unites its fragment root with that of every cell
 * of its class and another region (atomicMin on the links; rows do not wrap); every fragment root finds its group root
 * and adds its size there; every pixel takes its group's root and count.  Integer atomics only: apart from the record
 * order the outputs are a function of the inputs alone.  Any h, w >= 1; n < 65536, n h w <= 2^31 - 1,
 * 2 <= num_classes <= 255 and image_base + n <= 2^31 - 1, else UNET_ERR_UNSUPPORTED (and the workspace query returns 0);
 * gap outside 1..32, min_pixels < 1, a negative image_base or capacity or a NULL pointer is UNET_ERR_BAD_ARG; all of
 * that before any launch.  Allocates nothing, does not synchronise. */
size_t unet_group_class_regions_workspace(int64_t n, int64_t h, int64_t w, int32_t num_classes);
int32_t unet_group_class_regions(const uint8_t* classes, const int32_t* region, const int32_t* sizes, int64_t n,
                                 int64_t h, int64_t w, int32_t num_classes, int32_t gap, int32_t min_pixels,
                                 int32_t image_base, int32_t* group, int32_t* group_sizes, int64_t* counts,
                                 int64_t* fragments, int64_t capacity, int64_t* fragment_count, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* Overlaps of region pairs (no reference counterpart: the sparse contingency table between two region labellings, from
 * which detection against a confidence threshold, "found with the wrong class" and IoU matching are host arithmetic).
 * truth_region / pred_region: two `region` arrays of unet_label_class_regions, int32 [n][h][w], 1 + root index, 0 on
 * background.  A pixel carries the pair (truth id, pred id) iff both are positive, whatever the regions' classes.  The
 * ids are compared and packed, never used as an index.
 * unet_region_pair_bound: bound[n] (int64, device; ADDED to: zero it first) += the pixels of image n that carry a pair
 * and have x == 0 or another pair (or none) to their left.  The row-major first pixel of every distinct pair is one of
 * them, so bound[n] >= the distinct pairs of image n.
 * unet_region_pairs: one record of 4 int32 {image_base + image, truth id - 1, pred id - 1, overlap} per distinct pair of
 * every image, overlap = the pixels that carry it, at the slot that an atomic add on count[1] (int64, device; ADDED to:
 * zero it first) hands out: the order is arbitrary, sort by (image, truth root, pred root).  record_cap = records that
 * the buffer holds; a record past it is counted and not written.  The pairs of an image are counted in an
 * open-addressing table of `capacity` slots (a power of two, else UNET_ERR_BAD_ARG) in the workspace (8-byte aligned),
 * which the call clears: key = truth id << 32 | pred id (0 = empty), atomicCAS on the key, integer atomicAdd on the
 * slot's count, linear probing for at most `capacity` steps.  A pixel that finds no slot is dropped and adds 1 to
 * overflow[1] (int64, device; ADDED to: zero it first): with overflow == 0 and count <= record_cap the records are
 * complete, which capacity >= bound[n] for every n and record_cap >= their sum guarantee; the pairs that did find a
 * slot have their full overlap either way.  Integer atomics only: the set of records is a function of the two maps alone.
 * Any h, w >= 1; n < 65536, n h w <= 2^31 - 1, capacity <= 2^30, n capacity <= 2^40, image_base + n and record_cap
 * <= 2^31 - 1, else UNET_ERR_UNSUPPORTED before any launch (and the workspace query returns 0, as for a capacity that is
 * no power of two).  Allocate nothing, do not synchronise. */
int32_t unet_region_pair_bound(const int32_t* truth_region, const int32_t* pred_region, int64_t n, int64_t h, int64_t w,
                               int64_t* bound /* [n] */, void* stream);
size_t unet_region_pairs_workspace(int64_t n, int64_t capacity);
int32_t unet_region_pairs(const int32_t* truth_region, const int32_t* pred_region, int64_t n, int64_t h, int64_t w,
                          int64_t capacity, int32_t image_base, int32_t* records, int64_t record_cap, int64_t* count,
                          int64_t* overflow, void* workspace, size_t workspace_bytes, void* stream);

/* Per-defect records of class regions (no reference counterpart: what a predicted defect is on its own terms -- where,
 * how large, how sure the model was -- for images that have no ground truth).  classes, region and sizes are what
 * unet_label_class_regions takes and makes; conf: fp32 [n][h][w], the per-pixel confidence of unet_seg_confidence, or
 * NULL.  Every region with size >= min_pixels (>= 1) yields one record of 12 int64 {image_base + image, class, root
 * index y * w + x, size, x0, y0, x1, y1, sum_x, sum_y, conf_sum_q, conf_max_q}: the inclusive bounding box, the sums of
 * the pixels' coordinates (centroid = sum / size), and the sum and the maximum over the region's pixels of
 * q(v) = (uint32) rint(v * 65536.0f) (ties to even) on v clamped to [0, 1]; finite conf only; both 0 with conf == NULL.
 * The slot comes from an atomic add on record_count[1] (int64, device; ADDED to: zero it first): the order is arbitrary,
 * sort by (image, root index).  capacity = records that the buffer holds (<= 2^31 - 1); a record past it is counted and
 * not written.  Two launches: the root pixels take their slots (one atomic per block), write their own pixel's values
 * as the record and leave the slot in the workspace, then every other class pixel folds its values into its region's
 * record with integer atomicMin / atomicMax / atomicAdd -- summed in registers, across the wave and across the block
 * first where the pixels share a region, so a large region costs one atomic per field and block.  Integer atomics only:
 * apart from the record order the output is a function of the inputs alone (that is why the confidence is summed in
 * fixed point).  Any h, w >= 1; n < 65536,
 * n h w <= 2^31 - 1, 2 <= num_classes <= 255, image_base + n and capacity <= 2^31 - 1, else UNET_ERR_UNSUPPORTED before
 * any launch (and the workspace query returns 0); min_pixels < 1 is UNET_ERR_BAD_ARG.  Allocates nothing, does not
 * synchronise. */
size_t unet_describe_class_regions_workspace(int64_t n, int64_t h, int64_t w, int32_t num_classes);
int32_t unet_describe_class_regions(const uint8_t* classes, const int32_t* region, const int32_t* sizes,
                                    const float* conf /* [n][h][w], may be NULL */, int64_t n, int64_t h, int64_t w,
                                    int32_t num_classes, int32_t min_pixels, int32_t image_base, int64_t* records,
                                    int64_t capacity, int64_t* record_count, void* workspace, size_t workspace_bytes,
                                    void* stream);

/* Shape records of class regions (no reference counterpart; csrc/shapes.hip, restated in numpy by tests/_shapes_ref.py):
 * what a defect's length, width, orientation, perimeter and holes are computed from.  region and sizes are what
 * unet_label_class_regions makes (region[g] - 1 = the root of pixel g, 0 = background).  direction_table: HOST int32
 * [directions][2], the vectors (c_k, s_k), read during the call and passed to the kernels by value; every component in
 * -16384..16384 (else UNET_ERR_BAD_ARG).  Every region with size >= min_pixels (>= 1) yields one record of
 * 11 + 2 directions int64 {image_base + image, root index y * w + x, size, sum_xx, sum_yy, sum_xy, q1, q2, qd, q3, q4,
 * pmin_0 .. pmin_{D-1}, pmax_0 .. pmax_{D-1}}: the sums of x x, y y and x y over the region's pixels in frame
 * coordinates; the bit-quad counts (Gray 1971) over all (h + 1)(w + 1) 2 x 2 windows of the region's own mask padded
 * with non-members -- windows with one member, two edge-adjacent, two diagonal, three and four; a pixel of another
 * region or class or outside the frame is a non-member --; and the minimum and maximum of x c_k + y s_k over the
 * region's pixels.  Slots, record_count (ADDED to: zero it first), capacity and the record order are those of
 * unet_describe_class_regions: with equal min_pixels and image_base the two calls keep the same regions, and sorted by
 * (image, root index) their records align.  Two launches: the root pixels take their slots and write their own pixel's
 * values, leaving the slot in the workspace (all of it is written); every other class pixel adds its moments and the
 * windows it is the first member of (summed per thread, wave and block first) with int64 atomicAdd, and, if one of its 8
 * neighbours is a non-member, its projections with atomicMin / atomicMax (reduced across the wave first, and only
 * issued where they improve on the record).  Integers only: apart from the record order the output is a function of the
 * inputs alone.  n < 65536, n h w <= 2^31 - 1, h and w <= 16384 (sum_xx <= 2^56, |p| < 2^30), directions even in
 * 2..32, image_base + n and capacity <= 2^31 - 1, else UNET_ERR_UNSUPPORTED before any launch (and the workspace query
 * returns 0); a NULL pointer or min_pixels < 1 is UNET_ERR_BAD_ARG.  Allocates nothing, does not synchronise. */
size_t unet_measure_class_regions_workspace(int64_t n, int64_t h, int64_t w, int32_t directions);
int32_t unet_measure_class_regions(const int32_t* region, const int32_t* sizes, int64_t n, int64_t h, int64_t w,
                                   int32_t min_pixels, int32_t image_base,
                                   const int32_t* direction_table /* host [directions][2] */, int32_t directions,
                                   int64_t* records, int64_t capacity, int64_t* record_count, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* Outlines of class regions (no reference counterpart; csrc/contours.hip, restated one edge at a time by
 * tests/_contours_ref.py): the inverse of unet_polygon_mask_u8, each kept region's boundary as pixel-centre polygons.
 * region and sizes are what unet_label_class_regions makes; a region is kept iff its size >= min_pixels (>= 1), the rule
 * of unet_describe_class_regions.  A directed crack edge is (pixel p, direction d), d = 0 E (+x), 1 S (+y), 2 W, 3 N: it
 * exists when p is a pixel of a kept region and its neighbour in direction r = (d + 1) % 4 is not a pixel of that region
 * (outside the frame counts), and its id is 4 (y w + x) + d.  Its successor is (p + d + r, r) if that pixel is a member,
 * else (p + d, d) if that one is, else (p, (d + 3) % 4); the edges fall into loops.  A loop's leader is its smallest id;
 * area2 = the sum over its edges of x1 y0 - x0 y1 between their pixel-corner end points: +2 for one pixel, > 0 for a
 * region's one outer loop, < 0 for each hole loop.  Its points: the edges' pixels in walk order from the leader, cyclic
 * repeats merged, every point dropped whose step in equals its step out (a loop around one pixel keeps that pixel).
 * unet_count_class_region_edges: counts[3] (int64, device, WRITTEN) = {edges, loops, points} of the maps, one pass over
 * the pixels and no tracing (loops = twice the kept regions minus the Euler numbers of their masks).
 * unet_trace_class_regions: counts as above, and for edges <= edge_cap: loops[L][6] (int64) = {image_base + image, region
 * root index y w + x, leader edge id, n_points, first point, area2} in ascending (image, leader edge id), and
 * points[P][2] (int32) = (x, y), each loop's points contiguous from its first point.  A row at or past loop_cap and a
 * point at or past point_cap are not written; with edges > edge_cap nothing is; the counts are the true ones either way.
 * Every position is a prefix sum and area2 an integer atomic add: the outputs are a function of the inputs alone, byte
 * for byte.  The edges are compacted, a loop's leader and every edge's point ordinal are found by pointer doubling, one
 * launch per round over ping-pong buffers, ceil(log2(edge_cap)) rounds each.
 * Both: any h, w >= 1; n < 65536 and n h w <= 2^29 (an edge id fits int32); image_base + n, edge_cap, loop_cap and
 * point_cap <= 2^31 - 1; else UNET_ERR_UNSUPPORTED before any launch (and the workspace queries return 0).  A NULL
 * pointer (loops / points may be NULL with a capacity of 0) or min_pixels < 1 is UNET_ERR_BAD_ARG.  Allocate nothing, do
 * not synchronise. */
size_t unet_count_class_region_edges_workspace(int64_t n, int64_t h, int64_t w);
int32_t unet_count_class_region_edges(const int32_t* region, const int32_t* sizes, int64_t n, int64_t h, int64_t w,
                                      int32_t min_pixels, int64_t* counts /* [3] */, void* workspace,
                                      size_t workspace_bytes, void* stream);
size_t unet_trace_class_regions_workspace(int64_t n, int64_t h, int64_t w, int64_t edge_cap);
int32_t unet_trace_class_regions(const int32_t* region, const int32_t* sizes, int64_t n, int64_t h, int64_t w,
                                 int32_t min_pixels, int32_t image_base, int64_t edge_cap, int64_t* loops,
                                 int64_t loop_cap, int32_t* points, int64_t point_cap, int64_t* counts /* [3] */,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* Outline accuracy of label maps (no reference counterpart): an exact squared Euclidean distance transform of the class
 * boundaries, and one record per (image, class) of how far the outlines of two maps lie apart (csrc/distance.hip).
 * classes / truth / pred: uint8 [n][h][w] as unet_label_class_regions takes them; a pixel has class c iff its value is c,
 * 1 <= c < num_classes.  A pixel of class c is a boundary pixel of c iff at least one of its 4-neighbours INSIDE the frame
 * has another value: the frame edge makes no boundary, so a class that covers the frame or is absent has none.
 * unet_boundary_distance_sq: d2_out (int32 [n][num_classes - 1][h][w]) = the minimum of (y - y')^2 + (x - x')^2 over the
 * boundary pixels (y', x') of class c of image n at [n][c - 1][y][x], UNET_BOUNDARY_NONE everywhere in a plane whose image
 * has no boundary pixel of the class.  Two launches: columns (vertical distance, all classes from one read of the labels),
 * then rows in place (a workgroup per row, the row in LDS, an outward search that stops once dx^2 reaches the best
 * value).  The workspace (4-byte aligned) holds one flag per (image, class); the call clears it.
 * unet_boundary_stats: records (int64 [n][num_classes - 1][UNET_BOUNDARY_FIELDS], ADDED to: zero them first) = {image_base
 * + image, class, t_pixels, p_pixels, t_boundary, p_boundary, p_near[4], t_near[4], band_inter, band_union, p_dist_sum_q8,
 * t_dist_sum_q8, p_dist_max_sq, t_dist_max_sq}: pixels and boundary pixels of the class in truth and prediction;
 * p_near[i] = predicted boundary pixels with d2_truth <= tol_sq[i] and t_near[i] = truth boundary pixels with d2_pred <=
 * tol_sq[i] (tol_sq: HOST array of k <= 4 values, the slots from k on stay 0); band_inter / band_union = intersection and
 * union of {truth pixels of the class with d2_truth <= band_sq} and {predicted pixels of the class with d2_pred <=
 * band_sq}; the sums over a map's boundary pixels of dist_q8 = floor(256 sqrt(d2)) (exact: isqrt(d2 << 16)) of the OTHER
 * map's d2, and the maxima of that d2.  A boundary pixel whose other map has no boundary of the class (d2 ==
 * UNET_BOUNDARY_NONE) adds to t_boundary / p_boundary only.  hist (int64 [num_classes - 1][2][1025], ADDED to): direction
 * 0 = prediction to truth, 1 = truth to prediction, bin min(isqrt(d2), 1024), from the boundary pixels that feed the
 * sums.  d2_truth / d2_pred: what unet_boundary_distance_sq made of truth / pred.  Integer atomics only (per block in LDS,
 * then 64-bit atomicAdd / atomicMax): the outputs are a function of the two maps alone.
 * Both: 1 <= h, w <= 4096, 2 <= num_classes <= 32, n < 65536, n (num_classes - 1) h w < 2^31 (and image_base + n <=
 * 2^31 - 1), else UNET_ERR_UNSUPPORTED before any launch (and the workspace query returns 0); k outside 0..4 or a tol_sq /
 * band_sq outside 0 .. 2^30 - 1 is UNET_ERR_BAD_ARG.  Allocate nothing, do not synchronise. */
#define UNET_BOUNDARY_NONE (1 << 30)
#define UNET_BOUNDARY_FIELDS 20
size_t unet_boundary_distance_sq_workspace(int64_t n, int64_t h, int64_t w, int32_t num_classes);
int32_t unet_boundary_distance_sq(const uint8_t* classes, int64_t n, int64_t h, int64_t w, int32_t num_classes,
                                  int32_t* d2_out, void* workspace, size_t workspace_bytes, void* stream);
int32_t unet_boundary_stats(const uint8_t* truth, const uint8_t* pred, const int32_t* d2_truth, const int32_t* d2_pred,
                            int64_t n, int64_t h, int64_t w, int32_t num_classes, const int32_t* tol_sq /* host [k] */,
                            int32_t k, int32_t band_sq, int32_t image_base, int64_t* records, int64_t* hist, void* stream);

/* AUPRO: the area below the per-region-overlap curve up to a false-positive rate of fpr_limit, divided by fpr_limit (the
 * localisation metric of the MVTec AD evaluation; no reference counterpart).  With R regions and N ok pixels, walking
 * the distinct scores v downwards from the point (0, 0): fpr = #{ok pixels >= v} / N, pro = sum over the defective
 * pixels >= v of 1 / (R * size of the pixel's region); the curve is piecewise linear through these points and the
 * segment that crosses fpr_limit is cut there by interpolation.  Two steps, as unet_rank_auc:
 * unet_region_auc_append: over the images with select[n] != 0 (NULL: all) of pred (fp32) / sizes (int32, of
 * unet_label_regions), both [n_images][per_image]: every finite score becomes an order-preserving uint32 key
 * (-0.0 == +0.0).  slots is capacity 8-byte slots: a defective pixel (sizes > 0) is written as the uint64 element
 * key << 32 | size to slot counts[0] ... upwards, an ok pixel as a uint32 key to the uint32 entry
 * 2 capacity - 1 - counts[1] ... downwards, in no particular order; counts[3] = {defective, ok, non-finite scores}
 * (int64, device) is ADDED to: zero it first, and size capacity >= every selected pixel of every call that adds to the
 * same counts.  Integer atomics only; allocates nothing, does not synchronise.
 * unet_region_auc: sorts pos_pairs[n_pos] (on all 64 bits: every size must be <= max_region) and neg_keys[n_neg] (LSD
 * radix sort; 16-byte aligned arrays, contents destroyed) and writes out[2] (fp64, device) = {AUPRO, pro at fpr_limit}.
 * regions = R; 0 < fpr_limit <= 1.  n_pos == 0, n_neg == 0 or regions == 0: {0, 0}.  Non-finite scores are the
 * caller's to handle.  n_pos + n_neg >= 2^31 is UNET_ERR_UNSUPPORTED (and the workspace query returns 0).  Ordered
 * fp64 sums over the sorted arrays, no float atomics: the result depends only on the multiset of (score, region size)
 * pixels, bitwise. */
int32_t unet_region_auc_append(const float* pred, const int32_t* sizes, const uint8_t* select, int64_t n_images,
                               int64_t per_image, void* slots, int64_t capacity, int64_t* counts, void* stream);
size_t unet_region_auc_workspace(int64_t n_pos, int64_t n_neg);
int32_t unet_region_auc(uint64_t* pos_pairs, int64_t n_pos, uint32_t* neg_keys, int64_t n_neg, int64_t regions,
                        int64_t max_region, double fpr_limit, double* out, void* workspace, size_t workspace_bytes,
                        void* stream);

/* The visualisation sheet of the evaluation CLI (src/test.py:315-332 -> src/utils.py:111-157 visualize_results, drawn
 * there by matplotlib on the host): n rows of k <= 8 panels of h x w pixels as one packed uint8 RGB image
 * sheet[n h + (n - 1) gutter][k w + (k - 1) gutter][3], panels separated by `gutter` pixels of 255 in both directions.
 * panels: HOST array of k descriptions, one per column; rgb = fp32 [n][3][h][w], map = fp32 [n][1][h][w] (device):
 *   UNET_PANEL_IMAGE    rgb, ImageNet-normalised: v = x * std3[c], then + mean3[c] (fp32, each rounded), clamped to
 *                       [0, 1]; byte = (uint8)(v * 255.0f), truncating; NaN gives 0
 *   UNET_PANEL_UNIT     rgb in [0, 1]: the clamp and the byte rule alone (the reconstruction)
 *   UNET_PANEL_GRAY     map through a 256-entry colour table after scaling the plane to its own range, in fp64:
 *   UNET_PANEL_HOT      t = ((double)x - lo) / (hi - lo), i = floor(256 t) clipped to [0, 255]; hi == lo gives i = 0;
 *                       lo / hi = the smallest / largest finite value of the plane; a non-finite pixel, and every pixel
 *                       of a plane without a finite one, is (255, 255, 255).  The index is the one matplotlib's
 *                       cmap(Normalize()(x.astype(float64))) takes, exactly
 *   UNET_PANEL_OVERLAY  rgb and map: (alpha8 * HOT(map) + (255 - alpha8) * IMAGE(rgb) + 127) / 255 per channel in
 *                       integers, 0 <= alpha8 <= 255; a non-finite map pixel shows the image
 * Two steps.  The range step writes keys[2][k][n] (uint32, device): the order-preserving keys (as in the rank-AUC
 * append step, -0.0 == +0.0) of lo, then of hi, of every map plane; a plane without a finite pixel keeps lo = 0xffffffff
 * > hi = 0; entries of panels without a map are not read.  Integer atomicMin / atomicMax only: independent of scheduling.
 * The sheet step takes those keys and luts[2][256][3] (device bytes: the gray table, then the hot one) and writes the
 * whole sheet in one launch.  mean3 / std3 are HOST arrays.  Any h, w >= 1 and gutter >= 0; k > 8, n >= 65536 or a sheet
 * of 2^31 bytes or more is UNET_ERR_UNSUPPORTED.  Allocates nothing, does not synchronise. */
enum unet_panel_kind {
  UNET_PANEL_IMAGE = 0, UNET_PANEL_UNIT = 1, UNET_PANEL_GRAY = 2, UNET_PANEL_HOT = 3, UNET_PANEL_OVERLAY = 4
};
typedef struct unet_panel {
  int32_t kind;        /* unet_panel_kind */
  int32_t alpha8;      /* UNET_PANEL_OVERLAY only */
  const float* rgb;
  const float* map;
} unet_panel;
int32_t unet_render_range(const unet_panel* panels, int32_t k, int32_t n, int32_t h, int32_t w, uint32_t* keys,
                          void* stream);
int32_t unet_render_sheet(const unet_panel* panels, int32_t k, int32_t n, int32_t h, int32_t w, int32_t gutter,
                          const float* mean3, const float* std3, const uint32_t* keys, const uint8_t* luts,
                          uint8_t* sheet, void* stream);

/* Per-pixel prediction and confidence of the Gear / KolektorSDD visualisation CLIs (visualize.py:134-135,
 * visualize_kolektorsdd.py:131: softmax(logits, dim=0).max(dim=0)[0]; torch.argmax) of fp32 NCHW logits [n][c][hw],
 * 2 <= c <= 8 (the limits of unet_seg_image_stats): labels[n][hw] (uint8) = argmax over classes, the FIRST maximum winning
 * ties (as torch.argmax and unet_seg_image_stats); conf[n][hw] (fp32) = 1 / sum_j expf(z_j - max z), every operation in
 * fp32, j in class order.  labels or conf may be NULL (not both).  The contract covers finite logits.  One streaming
 * launch: a lane owns 4 consecutive pixels (16-byte loads and stores) when hw % 4 == 0 and the pointers are aligned
 * (logits, conf 16 bytes; labels 4), else one pixel -- with hw % 4 != 0 the class planes of a pixel do not share an
 * alignment, so such shapes run on scalar accesses throughout.  Other c, n < 1 or hw < 1: UNET_ERR_UNSUPPORTED.
 * Allocates nothing, does not synchronise. */
int32_t unet_seg_confidence(const float* logits, int32_t n, int32_t c, int64_t hw, uint8_t* labels, float* conf,
                            void* stream);

/* Calibration of that confidence (no reference counterpart; csrc/calibration.hip, restated in numpy by
 * tests/_calibration_ref.py): the confidence at a temperature, a reliability histogram, and the negative log-likelihood
 * at up to 32 temperatures from one read of the logits.  All three refuse on the host, before any HIP call and so also
 * without a GPU, with UNET_ERR_UNSUPPORTED (-2, the status unet_seg_confidence gives for its class count): a NULL
 * pointer, c outside 2..8, n < 1, hw < 1 (histogram and sweep: hw > 2^31 - 1; sweep: n >= 65536), bins outside 1..64, k
 * outside 1..32, select not 0 or 1, an inv_t that is not a finite fp32 > 0.  They allocate nothing and do not synchronise.
 *
 * unet_seg_confidence_scaled: unet_seg_confidence of softmax(z / T), inv_t = 1 / T.  labels = the first maximum of the RAW
 * logits (a rounding of z * inv_t can never change a label); conf = 1 / sum_j expf((z_j - max z) * inv_t), every
 * operation one fp32 rounding, j in class order.  The same 16-byte / scalar access rule.  At inv_t == 1.0f the product is
 * exact and the bytes are those of unet_seg_confidence.  labels or conf may be NULL (not both).
 *
 * unet_reliability_histogram: labels (uint8) and conf (fp32) as unet_seg_confidence_scaled or unet_tile_blend wrote them,
 * target (int64), all [n][hw].  hist (uint64 [c][bins][3], device, ADDED to: zero it first): per PREDICTED class and
 * confidence bin {pixels, pixels whose target equals the label, sum of q}, q(v) = (uint32) rint(v * 65536.0f) (ties to
 * even) on v clamped to [0, 1], NaN -> 0 (the rule of unet_describe_class_regions), bin = min(bins - 1, (q * bins) >> 16).
 * A pixel is skipped, and counted in skipped[0] (uint64, device, ADDED to), when its target is ignore_index or outside
 * 0..c-1 or its label is >= c.  select 0 takes every other pixel, select 1 only those whose target or label is not class
 * 0; a pixel that select leaves out is not counted anywhere.  Integers only (32-bit LDS cells per block of at most 4096
 * pixels, 64-bit integer atomics to memory): the outputs are a function of the inputs alone, and no cell overflows before
 * 2^47 pixels.
 *
 * unet_temperature_sweep: logits fp32 [n][c][hw], target int64 [n][hw], inv_t = HOST array of k values.  With d_j = z_j -
 * max z and t the target: nll[i] (fp64 [k], device, ADDED to) += the sum over the pixels taken of
 * logf(sum_j expf(d_j * inv_t[i])) - d_t * inv_t[i], the per-pixel term in fp32 with every product and sum rounded once
 * (j in class order), the sum in fp64.  counted (uint64 [2], device, ADDED to): [0] the pixels taken, [1] the pixels with a
 * non-finite logit, which are set aside first, whatever their target.  The skip and select rules are the histogram's,
 * with the label = the first maximum, computed here.  The order of summation is a function of (n, hw, k) alone (fixed
 * pixel ranges per lane and block, shuffle trees, block partials in the workspace, one ordered final sum; no
 * floating-point atomics): two calls on the same input give the same bits, whichever of the 16-byte (hw % 4 == 0, aligned
 * pointers) and scalar loads they use.  The workspace (8-byte aligned) holds the block partials; too small a one is
 * UNET_ERR_WORKSPACE, and the query returns 0 for a shape the call refuses. */
int32_t unet_seg_confidence_scaled(const float* logits, int32_t n, int32_t c, int64_t hw, float inv_t, uint8_t* labels,
                                   float* conf, void* stream);
int32_t unet_reliability_histogram(const uint8_t* labels, const float* conf, const int64_t* target, int32_t n, int64_t hw,
                                   int32_t c, int32_t bins, int64_t ignore_index, int32_t select, uint64_t* hist,
                                   uint64_t* skipped, void* stream);
size_t unet_temperature_sweep_workspace(int32_t n, int64_t hw, int32_t k);
int32_t unet_temperature_sweep(const float* logits, const int64_t* target, int32_t n, int32_t c, int64_t hw,
                               int64_t ignore_index, int32_t select, const float* inv_t /* host [k] */, int32_t k,
                               double* nll, uint64_t* counted, void* workspace, size_t workspace_bytes, void* stream);

/* The prediction sheets of the Gear / KolektorSDD visualisation CLIs (visualize.py:120-236 visualize_single_prediction /
 * visualize_prediction_grid, visualize_kolektorsdd.py:101-202, drawn there by matplotlib on the host) as one packed
 * uint8 RGB image written by one launch: R = ceil(n / per_row) rows of per_row samples, each sample k <= 8 panels of
 * h x w pixels side by side; sample i sits in row i / per_row at cell i % per_row.
 * sheet[R h + (R - 1) gutter][per_row k w + (per_row k - 1) gutter][3]; the gutters and the cells past n are 255.
 * image = fp32 [n][3][h][w], ImageNet-normalised (device; may be NULL when no panel draws it).  panels: HOST array of k
 * descriptions; labels = uint8 [n][h][w], map = fp32 [n][h][w] (device):
 *   UNET_SEG_PANEL_IMAGE    the bytes of UNET_PANEL_IMAGE: v = x * std3[c], then + mean3[c] (fp32, each rounded), clamped
 *                           to [0, 1], NaN gives 0; byte = (uint8)(v * 255.0f), truncating
 *   UNET_SEG_PANEL_CLASSES  palette[labels[p]] (imshow(mask, cmap='tab10', ...), visualize_kolektorsdd.py:118-124)
 *   UNET_SEG_PANEL_OVERLAY  where labels[p] == 0 the IMAGE byte (no overlay on the background, visualize.py:112-113),
 *                           elsewhere (alpha8 * palette[l] + (255 - alpha8) * IMAGE + 127) / 255 per channel in integers,
 *                           0 <= alpha8 <= 255: the blend of UNET_PANEL_OVERLAY.  This is the library's own blend; it is
 *                           NOT claimed to equal Agg's compositing of the reference's RGBA layer (visualize.py:102-117)
 *   UNET_SEG_PANEL_LUT      map over the fixed range [0, 1] (imshow(vmin=0, vmax=1), visualize_kolektorsdd.py:132):
 *                           lut[min(floor(v * 256), 255)] for finite v, v < 0 gives lut[0]; a non-finite pixel is
 *                           (255, 255, 255), like the map panels of unet_render_sheet
 * palette[256][3] and lut[256][3] are device bytes; mean3 / std3 are HOST arrays.  Any h, w >= 1, gutter >= 0 and
 * per_row >= 1 (pixels are packed into whole 32-bit stores where the row allows, byte stores elsewhere); k > 8,
 * n >= 65536 or a sheet of 2^31 bytes or more is UNET_ERR_UNSUPPORTED.  The bytes are a function of the inputs alone.
 * Allocates nothing, does not synchronise. */
enum unet_seg_panel_kind {
  UNET_SEG_PANEL_IMAGE = 0, UNET_SEG_PANEL_CLASSES = 1, UNET_SEG_PANEL_OVERLAY = 2, UNET_SEG_PANEL_LUT = 3
};
typedef struct unet_seg_panel {
  int32_t kind;        /* unet_seg_panel_kind */
  int32_t alpha8;      /* UNET_SEG_PANEL_OVERLAY only */
  const uint8_t* labels;
  const float* map;
} unet_seg_panel;
int32_t unet_seg_render_sheet(const float* image, const unet_seg_panel* panels, int32_t k, int32_t n, int32_t h,
                              int32_t w, int32_t gutter, int32_t per_row, const float* mean3, const float* std3,
                              const uint8_t* palette, const uint8_t* lut, uint8_t* sheet, void* stream);

/* ---- nn.Dropout2d of SegmentationUNet's bottleneck (src/model.py:129,146): y = x * scale[n][c] on dense NHWC; the
 * caller draws scale = bernoulli(1-p)/(1-p) per (image, channel); the same call is the backward (dx = dy * scale). */
int32_t unet_channel_scale(int32_t dtype, const void* x, const float* scale, int32_t n, int64_t hw, int32_t c, void* y,
                           void* stream);
/* ---- compute_anomaly_score (src/utils.py:205-215): score[n][hw] = mean_c (recon - image)^2 (l1 != 0: mean_c |.|)
 * over fp32 NCHW planes, image_score[n] = mean over pixels (ordered partials). */
size_t unet_anomaly_score_workspace(int32_t n, int64_t hw);
int32_t unet_anomaly_score(const float* recon, const float* image, int32_t n, int32_t c, int64_t hw, int32_t l1,
                           float* score, float* image_score, void* workspace, size_t workspace_bytes, void* stream);

/* ---- input pipeline on the GPU: transforms.ToTensor() + Normalize(mean, std) (+ the training
 * RandomHorizontalFlip) of src/dataset.py:134-146 / src/kolektorsdd_dataset.py:133-150 for a batch of decoded uint8
 * images [n][h][w][3] (device memory): out[n][c][y][x] = (u8 / 255 - mean[c]) / std[c], mirrored in x where flip[n] != 0
 * (flip may be NULL; mean3 / std3 are HOST arrays).  The same fp32 operations in the same order: bit-identical. */
int32_t unet_preprocess_u8(const uint8_t* images_hwc, const uint8_t* flip, float* out_nchw, int32_t n, int32_t h,
                           int32_t w, const float* mean3, const float* std3, void* stream);

/* ---- the rest of the loaders' image transform on the GPU (round 4).  The reference runs torchvision on
 * PIL images (src/dataset.py:134-141: Resize -> RandomHorizontalFlip -> RandomRotation(10) -> ColorJitter(0.1, 0.1,
 * 0.1, 0.05) -> ToTensor -> Normalize; src/kolektorsdd_dataset.py:133-150: the same with RandomRotation(5), masks
 * Resize(NEAREST)); each entry point below restates the arithmetic of the Pillow C kernel that transform ends in and is
 * bit-exact against fixtures produced by PIL (tests/golden/aug_*.npz).  Batches are decoded uint8 images [n][h][w][c]
 * in device memory; the random draws stay with the host and come in as per-image parameters.
 *
 * transforms.Resize on a PIL image = Image.resize(BILINEAR) = ImagingResample (Resample.c): a separable triangle filter
 * whose support grows with the down-scale factor, 22-bit fixed-point coefficients, 8-bit intermediate image between the
 * horizontal and the vertical pass.  unet_resize_bilinear_coeffs (HOST function, host arrays) writes PIL's tables for
 * one axis: bounds[out][2] = (first source index, count), kk[out][ksize] with ksize = unet_resize_bilinear_ksize(..).
 * unet_resize_bilinear_u8 takes those tables in DEVICE memory (x tables for w -> out_w, y tables for h -> out_h; a pass
 * whose size does not change is skipped like PIL skips it and its tables may be NULL), tmp = [n][h][out_w][c] bytes
 * (needed when both passes run), c = 1 or 3. */
int32_t unet_resize_bilinear_ksize(int32_t in_size, int32_t out_size);
int32_t unet_resize_bilinear_coeffs(int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* kk);
int32_t unet_resize_bilinear_u8(const uint8_t* src, int32_t n, int32_t h, int32_t w, int32_t c, int32_t out_h,
                                int32_t out_w, const int32_t* xbounds, const int32_t* xkk, int32_t xksize,
                                const int32_t* ybounds, const int32_t* ykk, int32_t yksize, uint8_t* tmp, uint8_t* dst,
                                void* stream);
/* Image.resize(NEAREST) (Geometry.c ImagingScaleAffine; the mask transform of src/kolektorsdd_dataset.py:147-150 and
 * :116-117): unet_resize_nearest_index (HOST) writes the source index of every output position of one axis (-1 =
 * outside); unet_resize_nearest_u8 gathers with the y / x tables in DEVICE memory. */
int32_t unet_resize_nearest_index(int32_t in_size, int32_t out_size, int32_t* idx);
int32_t unet_resize_nearest_u8(const uint8_t* src, int32_t n, int32_t h, int32_t w, int32_t c, int32_t out_h,
                               int32_t out_w, const int32_t* yidx, const int32_t* xidx, uint8_t* dst, void* stream);
/* Gear label masks (reference src/gear_dataset.py:112-201 _create_mask_from_labelme, then :241-259 Resize(NEAREST)):
 * dst[n][out_h][out_w] = class of source pixel (yidx[n][i], xidx[n][j]) -- the highest-priority raw class (1 -> 2, then
 * 0 -> 1, then 2 -> 3; others ignored) with a polygon whose ImageDraw.polygon(xy, fill=1) covers it, else 0.  verts
 * [V][2] (x, y) integer pixel coordinates; polygon p owns verts[poly_offsets[p] .. poly_offsets[p+1]) (>= 3 vertices,
 * at most max_poly_vertices <= 512), raw class poly_class[p], image poly_image[p] (non-decreasing); src_hw[n] = source
 * (h, w); per-image index tables from unet_resize_nearest_index (identity tables = the full-resolution mask).  All
 * arrays in DEVICE memory; out_w <= 4096. */
int32_t unet_polygon_mask_u8(const int32_t* verts, const int32_t* poly_offsets, const int32_t* poly_class,
                             const int32_t* poly_image, int32_t n_polys, int32_t max_poly_vertices, const int32_t* src_hw,
                             int32_t n, int32_t out_h, int32_t out_w, const int32_t* yidx, const int32_t* xidx,
                             uint8_t* dst, void* stream);
/* Class-overlap census of Gear label sets (reference analyze_class_overlaps.py): hist[n][8] (int64, DEVICE),
 * hist[i][b] = number of pixels of image i, at its native src_hw[i] = (h, w), whose set of covering raw classes is
 * exactly b -- bit c of b is set when at least one class-c polygon covers the pixel (several polygons of one class are
 * OR-ed; classes outside 0..2 are skipped).  Coverage is unet_polygon_mask_u8's rule and code; the polygon arrays have
 * the same layout and limits.  max_h / max_w = the largest height / width in src_hw: the grid scans rows 0 .. max_h - 1
 * of every image (rows beyond an image's height add nothing) and max_w <= 4096, n <= 65535, max_poly_vertices <= 512,
 * else UNET_ERR_UNSUPPORTED; an image wider than max_w adds nothing.  hist is cleared on `stream` before the launch;
 * the bins of image i sum to h * w.  Integer atomics only: the result does not depend on scheduling. */
int32_t unet_polygon_class_histogram(const int32_t* verts, const int32_t* poly_offsets, const int32_t* poly_class,
                                     const int32_t* poly_image, int32_t n_polys, int32_t max_poly_vertices,
                                     const int32_t* src_hw, int32_t n, int32_t max_h, int32_t max_w, int64_t* hist,
                                     void* stream);
/* RandomHorizontalFlip + RandomRotation: dst = rotate(flip[n] ? mirror(src) : src) with Image.rotate(angle, NEAREST,
 * expand=False, fill 0) = Geometry.c affine_fixed in 16.16 fixed point.  matrices[n][6] (DEVICE, may be NULL: no
 * rotation) = {a0, a1, a2, a3, a4, a5} ALREADY in fixed point, a2 / a5 including the half-pixel terms (FIX(a[2] +
 * a[0]*0.5 + a[1]*0.5)); flip[n] DEVICE bytes, may be NULL.  src != dst; sides < 32768; c <= 4. */
int32_t unet_flip_rotate_u8(const uint8_t* src, int32_t n, int32_t h, int32_t w, int32_t c, const uint8_t* flip,
                            const int32_t* matrices, uint8_t* dst, void* stream);
/* ColorJitter + ToTensor + Normalize of RGB batches.  Per image: `order` = the permutation torchvision draws (entries:
 * 0 brightness, 1 contrast, 2 saturation, 3 hue, -1 = skip), the three ImageEnhance factors (Blend.c: float32, truncating)
 * and hue_shift = uint8(hue_factor * 255) added to H of Convert.c's integer HSV.  The contrast operation needs the mean
 * L of the image as it is at that point of the list: one integer-sum pass, then one pass that applies the list and
 * writes out[n][c][y][x] = (u8 / 255 - mean[c]) / std[c] (fp32 NCHW, as unet_preprocess_u8).  desc: DEVICE array of n
 * (NULL: no jitter, no workspace needed); mean3 / std3: HOST arrays. */
typedef struct unet_jitter_desc {
  int32_t order[4];
  float brightness, contrast, saturation;
  int32_t hue_shift;
} unet_jitter_desc;
size_t unet_color_jitter_workspace(int32_t n);
int32_t unet_color_jitter_normalize_u8(const uint8_t* images_hwc, int32_t n, int32_t h, int32_t w,
                                       const unet_jitter_desc* desc, const float* mean3, const float* std3,
                                       float* out_nchw, void* workspace, size_t workspace_bytes, void* stream);
/* Synthetic anomalies for the MVTec trainer (DRAEM / CutPaste style), one launch per batch: inside a smooth random mask
 * the clean image is blended with a shifted, channel-permuted image of the same batch.  There is no reference code for
 * this -- the reference trains on train/good alone, so its masks are all zero and its reconstruction target is the
 * network's input -- hence the definition is this library's own: it is written out at the top of csrc/synth.hip and
 * restated independently in tests/_synth_ref.py, which the kernel equals bit for bit (fp32, no contraction).
 * images / corrupted [n][3][h][w] fp32 (normalised, distinct buffers), masks_in [n][1][h][w] fp32 or NULL, masks_out
 * [n][1][h][w] = max(masks_in, m) with m in {0, 1}.  Per image (desc: DEVICE array of n; desc_host: the same n structs in
 * HOST memory, read before the launch to check them): m = apply && noise(seed, cells_y, cells_x) > threshold; where m,
 * corrupted[ch] = beta * x[ch] + one_minus_beta * images[src][perm(ch)][(y + shift_y) % h][(x + shift_x) % w], elsewhere
 * corrupted = x bit for bit.  perm 0..5 = the permutations of (0, 1, 2) in lexicographic order.  Tables (DEVICE):
 * ycell [7][h] int32 and ytf [7][2][h] fp32 = cell index, then fraction t and fade(t), of every row for 1, 2, .. 64 cells;
 * xcell / xtf the same for the columns; gradients [256][2] = (cos, sin)(2 pi k / 256).  c != 3, n, h, w < 1, a side >=
 * 32768, src outside the batch, cells not a power of two in 1..64, a shift outside the frame or perm outside 0..5:
 * UNET_ERR_UNSUPPORTED before any launch.  No atomics, no workspace, no synchronisation. */
typedef struct unet_synth_desc {
  int32_t apply;              /* 0 leaves the image (and its mask) as it is */
  uint32_t seed;
  int32_t cells_y, cells_x;
  float threshold;
  float beta, one_minus_beta; /* both set by the caller: nothing recomputes 1 - beta */
  int32_t src, shift_y, shift_x, perm;
  int32_t reserved;
} unet_synth_desc;
int32_t unet_synth_anomalies(const float* images, const float* masks_in, int32_t n, int32_t c, int32_t h, int32_t w,
                             const unet_synth_desc* desc, const unet_synth_desc* desc_host, const int32_t* ycell,
                             const float* ytf, const int32_t* xcell, const float* xtf, const float* gradients,
                             float* corrupted, float* masks_out, void* stream);

/* Smoothing of anomaly maps for the MVTec evaluation (test.py --map_sigma, --image_score map_max; no reference
 * counterpart: src/test.py:66-133 ranks the raw map), one kernel per batch (csrc/smooth.hip, restated in float64 by
 * tests/_smooth_ref.py).  src / dst: n contiguous fp32 planes of h x w, distinct and not overlapping.  dst = the separable
 * correlation of src along W, then along H, with the symmetric kernel taps[|k|], k = -radius .. radius; the border is
 * scipy's `reflect`, folded as often as needed (index i -> j = i mod 2L, then 2L - 1 - j if j >= L), so sides shorter
 * than the radius work, down to 1 x 1.  fp32 accumulation: taps[0] * x[0], then fma(taps[k], x[-k] + x[+k], .) for k =
 * 1 .. radius.  taps: HOST array of radius + 1 finite floats; they travel in the kernel arguments, so nothing is
 * allocated, copied or synchronised and the call can be captured.  image_max (DEVICE, n floats, or NULL): overwritten
 * (the caller initialises nothing) with the largest element written to each plane of dst, bit for bit; NaN if any
 * element of the plane is NaN.  It is filled on the stream ahead of the kernel and raised by integer atomics on the
 * float's own bits: the same result in every run.  Null src / dst / taps, a negative n, h, w or radius, a non-finite
 * tap, src == dst or overlapping buffers: UNET_ERR_BAD_ARG; radius > UNET_SMOOTH_MAX_RADIUS or n * h * w > 2^31 - 1:
 * UNET_ERR_UNSUPPORTED; all before anything is enqueued.  n == 0 or an empty plane: UNET_OK, nothing enqueued. */
#define UNET_SMOOTH_MAX_RADIUS 32
int32_t unet_smooth_maps(const float* src, float* dst, int64_t n, int32_t h, int32_t w, const float* taps,
                         int32_t radius, float* image_max, void* stream);

/* Full-resolution prediction (predict_tiled; no reference counterpart: visualize.py and the evaluators squeeze every
 * image into the trainer's frame): a frame of h x w is cut into ny x nx overlapping tiles of th x tw that the model runs
 * at its trained size, tile t = i * nx + j at origin (oy[i], ox[j]), and the tile logits are blended back into one label
 * map and one confidence map (csrc/tiles.hip, restated by tests/_tiles_ref.py).  oy[ny], ox[nx]: HOST arrays; they travel
 * in the kernel arguments, so nothing is allocated, copied or synchronised and the calls can be captured.  Each axis must
 * be a cover of the frame: the first origin 0, the last frame - tile, strictly increasing, no gap larger than the tile;
 * anything else is UNET_ERR_BAD_ARG, as is a NULL pointer, so no table can send a kernel outside the frame or the tile
 * buffer.  Both: 1 <= ny, nx <= 64, 1 <= th <= h, 1 <= tw <= w, h w <= 2^31 - 1, else UNET_ERR_UNSUPPORTED; every
 * refusal is decided on the host before any launch.  One launch each, no atomics, no workspace; a lane owns 4 consecutive
 * x (16-byte loads and stores) when w, tw and every ox[j] are multiples of 4 and the pointers are 16-byte aligned (labels:
 * 4), else one pixel.  Allocates nothing, does not synchronise.
 *
 * unet_tile_gather: frame fp32 [c][h][w] -> tiles fp32 [ny nx][c][th][tw], tiles[t][ch][ky][kx] = frame[ch][oy[i] + ky]
 * [ox[j] + kx], bit for bit; any c >= 1.
 *
 * unet_tile_blend: tiles = fp32 logits [ny nx][c][th][tw], 2 <= c <= 8 (the limits of unet_seg_confidence), ramps
 * 1 <= ramp_y, ramp_x <= 256.  Along an axis of tile length L with ramp B the weight of tile offset k is the integer
 * q(k) = min(k + 1, L - k, B); a tile weighs q_y q_x at a pixel.  Per pixel, over the covering tiles in ascending i, then
 * ascending j: wsum += q_y q_x in int32 and acc_c = acc_c + (float)(q_y q_x) * z_c from acc_c = 0, the product and the
 * sum each one fp32 rounding; blended[c][h][w] (fp32, may be NULL) = acc_c / (float)wsum, one conversion and one
 * correctly rounded division.  A pixel under exactly ONE tile takes that tile's logits unchanged, so a single tile over
 * the frame gives the bytes of unet_seg_confidence.  labels[h][w] (uint8) and conf[h][w] (fp32) follow from the blended
 * logits by unet_seg_confidence's rule: the first maximum wins, conf = 1 / sum_j expf(z_j - max z) in class order.  labels
 * or conf may be NULL (not both).  The outputs are a function of the inputs alone.  The contract covers finite logits. */
int32_t unet_tile_gather(const float* frame, int32_t c, int32_t h, int32_t w, int32_t th, int32_t tw, const int32_t* oy,
                         int32_t ny, const int32_t* ox, int32_t nx, float* tiles, void* stream);
int32_t unet_tile_blend(const float* tiles, int32_t c, int32_t th, int32_t tw, const int32_t* oy, int32_t ny,
                        const int32_t* ox, int32_t nx, int32_t h, int32_t w, int32_t ramp_y, int32_t ramp_x,
                        uint8_t* labels, float* conf, float* blended, void* stream);

/* View ensembling (predict_views, eval_views; no reference counterpart: the reference asks its model once per image): the
 * logits of n_views views of one image -- the image resized by a factor, possibly mirrored -- are brought back onto one
 * frame of h x w and reduced (csrc/views.hip, restated by tests/_views_ref.py).  views[n_views]: a HOST array; the
 * descriptors travel in the kernel arguments, so nothing is allocated, copied or synchronised and the call can be
 * captured.  View v: logits = DEVICE fp32 [c][h][w] of ITS h x w, flip_x / flip_y = 1 when the model saw the image
 * mirrored along x / y (the logits are those of the mirrored image) else 0.
 * Sampling, per axis, in integers: for output index i of an axis with N frame and M view samples
 *   p = floor(((2 i + 1) M 2^15) / N) - 2^15 in 64-bit integers, clamped to [0, (M - 1) 2^16]: (i + 1/2) M / N - 1/2 in
 *   16.16, the half-pixel-centre convention with edge clamp; i0 = p >> 16, f = p & 0xFFFF, i1 = min(i0 + 1, M - 1);
 *   M == N gives the tap i with fraction 0.  A flipped axis reads M - 1 - i0 and M - 1 - i1.
 * The value of a view at a pixel, with a00 .. a11 the samples at (y0 | y1, x0 | x1): top = ((float)(65536 - fx) a00 +
 * (float)fx a01) 2^-16, bot likewise from a10 and a11, val = ((float)(65536 - fy) top + (float)fy bot) 2^-16, every product
 * and every sum one fp32 rounding.  A view with the frame's size on BOTH axes is not interpolated: its logits are taken
 * unchanged, bits included.
 * Reduction, per pixel and class: acc_c starts as the first view's value and adds the others in ascending view order;
 * merged[c][h][w] (fp32) = acc_c / (float)n_views, one correctly rounded division.  labels[h][w] (uint8) and conf[h][w]
 * (fp32) follow from the merged logits by unet_seg_confidence's rule: the first maximum wins, conf = 1 / sum_j expf(z_j -
 * max z) in class order.  agreement[h][w] (uint8) = the number of views whose own first maximum over the classes of val
 * equals the merged label.  Logits are averaged, not probabilities: merged, labels and agreement are a function of the
 * inputs alone, with no expf between.  Each output may be NULL, not all of them.  The contract covers finite logits.
 * Refused on the host before any HIP call, all UNET_ERR_UNSUPPORTED: a NULL views array or a NULL logits pointer;
 * n_views outside 1..16; c outside 2..8; h, w or a view's h, w outside 1..16384; every output NULL; a flip that is not 0
 * or 1.  One launch, no atomics, no LDS, no workspace; a lane owns 4 consecutive x (16-byte stores, and 16-byte loads of
 * the views of the frame's own size, reversed under flip_x) when w is a multiple of 4 and merged, conf and those views
 * are 16-byte aligned (labels, agreement: 4), else one pixel.  Allocates nothing, does not synchronise. */
typedef struct unet_merge_view {
  const float* logits;
  int32_t h, w;
  int32_t flip_x, flip_y;
} unet_merge_view;
int32_t unet_view_merge(const unet_merge_view* views, int32_t n_views, int32_t c, int32_t h, int32_t w, float* merged,
                        uint8_t* labels, float* conf, uint8_t* agreement, void* stream);

/* Affine crops of a ragged batch (train_gear_crops; no reference counterpart: the reference trains on squeezed frames):
 * n_crops crops of out_h x out_w, cut with scale, rotation and flip out of n_images images of DIFFERENT sizes, in one
 * launch (csrc/crops.hip, restated in numpy int64 by tests/_crops_ref.py).  src: one packed byte buffer of src_bytes
 * bytes; image i is [h][w][c] bytes at src + src_offset[i] with (h, w) = src_hw[i] ([n_images][2]); c is 1 or 3.
 * desc[k]: the image of crop k and its matrix {a0 .. a5} in 16.16 fixed point, a2 / a5 ALREADY holding the half-pixel
 * terms (the convention of the flip / rotate kernel above).  dst: [n_crops][out_h][out_w][c].  src, src_offset, src_hw,
 * desc and dst are DEVICE arrays.  mode 0 = nearest, 1 = bilinear; fill in 0..255.
 * Output pixel (y, x) of crop k, all in int64: u = a0 x + a1 y + a2, v = a3 x + a4 y + a5; nx = u >> 16, ny = v >> 16
 * (arithmetic shift: floor).  The pixel is inside iff 0 <= nx < w and 0 <= ny < h, in BOTH modes; outside every channel
 * is `fill`, so a mask cropped with the same matrix carries its ignore value exactly where the image carries fill.
 * Nearest: dst = src[ny][nx][ch].  Bilinear: ub = u - 32768, x0 = ub >> 16, fx = (ub & 0xFFFF) >> 8, x1 = x0 + 1, x0 and
 * x1 clamped to [0, w - 1]; the same along y; top = (256 - fx) p00 + fx p01, bot likewise from p10 and p11; dst =
 * ((256 - fy) top + fy bot + 32768) >> 16.  No floating point: the bytes are a function of the inputs alone, and a matrix
 * that maps pixel centres to pixel centres (unit scale, no rotation, flipped or not) copies bytes in both modes.
 * Whatever the device tables hold, the kernel stays inside src[0, src_bytes) and dst: a crop whose image is outside
 * 0..n_images-1, or whose image has src_offset < 0, a side <= 0 or src_offset + h w c > src_bytes, is written as all
 * `fill`, and every tap is clamped into its image.
 * Refused on the host before any launch: a NULL pointer (UNET_ERR_BAD_ARG); c not 1 or 3, mode not 0 or 1, fill outside
 * 0..255, out_h or out_w outside 1..4096, n_crops or n_images outside 1..65535, src_bytes <= 0 (UNET_ERR_UNSUPPORTED).
 * A lane stores one dword when out_w c is a multiple of 4 and dst is 4-byte aligned, else one byte.  Allocates nothing,
 * does not synchronise. */
typedef struct unet_crop_desc {
  int32_t image;
  int32_t a[6];
  int32_t reserved;
} unet_crop_desc;
int32_t unet_affine_crop_u8(const uint8_t* src, int64_t src_bytes, const int64_t* src_offset, const int32_t* src_hw,
                            int32_t n_images, int32_t c, const unet_crop_desc* desc, int32_t n_crops, int32_t out_h,
                            int32_t out_w, int32_t mode, int32_t fill, uint8_t* dst, void* stream);

/* Copy-paste crops (train_gear_paste; no reference counterpart; Ghiasi et al., CVPR 2021): the bilinear image crop and
 * the nearest mask crop of unet_affine_crop_u8 written together in ONE launch, with labelled defects of any image of the
 * batch pasted into them on the way out (csrc/paste.hip, restated in numpy int64 by tests/_paste_ref.py).
 * Buffers: images are 3-channel, packed exactly as for unet_affine_crop_u8 (src, src_bytes, src_offset, src_hw); mask i is
 * [h][w] bytes at masks + mask_offset[i] with the same (h, w) = src_hw[i], inside masks[0, mask_bytes).  desc[k] is crop
 * k as above.  paste_start is [n_crops + 1], ascending: crop k owns paste[paste_start[k] .. paste_start[k + 1] - 1],
 * applied in that order, so a later one lies on top; at most the first UNET_PASTE_MAX of them are looked at.  dst_image:
 * [n_crops][out_h][out_w][3]; dst_mask: [n_crops][out_h][out_w].  All are DEVICE arrays.  n_pastes may be 0, and paste
 * may then be NULL.
 * Output pixel (y, x) of crop k, all in int64:
 *  1. Base.  pix[ch] is the bilinear rule above on image desc[k].image with `fill`; lab is the nearest rule above on that
 *     image's mask with `ignore`; inside is that rule's inside.  With no pastes the two outputs are the bytes of the two
 *     unet_affine_crop_u8 launches.
 *  2. For each paste j of the crop, in order.  It is skipped when !inside (nothing is pasted onto fill), when (x, y) is
 *     outside dst, or when the donor image or its mask is not readable.  box is first intersected with the donor image.
 *     u = b0 x + b1 y + b2, v = b3 x + b4 y + b5; nx = u >> 16, ny = v >> 16.  member(px, py) is true iff (px, py) lies
 *     in the box and m = mask[py][px] has m != 0 && m != ignore.  If member(nx, ny): lab = mask[ny][nx].  The four
 *     bilinear taps and fx, fy are the crop rule's: ub = u - 32768, x0 = ub >> 16, x1 = x0 + 1, likewise y.  A tap is a
 *     member by its own position (x0 or x1, y0 or y1, BEFORE the clamp: a tap outside the donor image is never a
 *     member); its value is read at the clamped position.  w00 = (256 - fx)(256 - fy), w01 = fx (256 - fy), w10 =
 *     (256 - fx) fy, w11 = fx fy; alpha = the sum of w_ij over the member taps, 0..65536.  If alpha > 0: d[ch] = the
 *     crop rule's bilinear value of the donor image, pix[ch] = (alpha d[ch] + (65536 - alpha) pix[ch] + 32768) >> 16.
 * So: a paste matrix that maps pixel centres to pixel centres copies donor bytes and donor labels exactly where the
 * donor mask is set inside the box, and changes nothing elsewhere; the image gets a one-pixel soft edge (0 < alpha <
 * 65536 where member and other taps mix); the label is that of the donor pixel the image pixel mostly came from (the
 * nearest one); and dst_mask == ignore exactly where the base crop left its image.
 * Guards: the contract of unet_affine_crop_u8, per buffer.  Whatever the device tables hold, no load leaves
 * src[0, src_bytes) or masks[0, mask_bytes) and no store leaves the outputs.  A base image index outside 0..n_images-1
 * gives a crop of all `fill` / `ignore`; a base image that is not readable (src_offset < 0, a side <= 0, src_offset +
 * 3 h w > src_bytes) is all `fill`, a base mask that is not readable (the same test on mask_offset, h w, mask_bytes) all
 * `ignore`, and a crop with either takes no paste.  A paste whose donor index is outside 0..n_images-1, or whose donor
 * image or mask is not readable, is skipped, that paste only.  Paste indices are clamped into [0, n_pastes); a
 * paste_start that descends owns no paste.
 * Refused on the host before any launch: a NULL src, src_offset, src_hw, masks, mask_offset, desc, paste_start,
 * dst_image or dst_mask, or a NULL paste with n_pastes > 0 (UNET_ERR_BAD_ARG); n_pastes < 0, fill or ignore outside
 * 0..255, out_h or out_w outside 1..4096, n_crops or n_images outside 1..65535, src_bytes or mask_bytes <= 0
 * (UNET_ERR_UNSUPPORTED).
 * A block works on a segment of one output row of one crop, so every descriptor, guard and the test of the row and
 * segment against dst is wave-uniform.  When out_w is a multiple of 4 and both outputs are 4-byte aligned a lane owns 4
 * consecutive pixels and stores whole dwords (three for the image, one for the mask), else one pixel with byte stores.
 * No atomics, no LDS, no floating point.  Allocates nothing, does not synchronise. */
#define UNET_PASTE_MAX 8
typedef struct unet_paste_desc {   /* 64 bytes */
  int32_t image;      /* donor image */
  int32_t b[6];       /* crop pixel (x, y) -> donor source point, 16.16, b2 / b5 holding the half-pixel terms */
  int32_t box[4];     /* x0, y0, x1, y1, half-open, donor pixels: only donor pixels inside it can be members */
  int32_t dst[4];     /* x0, y0, x1, y1, half-open, crop pixels: the paste is looked at only inside it */
  int32_t reserved;
} unet_paste_desc;
int32_t unet_paste_crop_u8(const uint8_t* src, int64_t src_bytes, const int64_t* src_offset, const int32_t* src_hw,
                           int32_t n_images, const uint8_t* masks, int64_t mask_bytes, const int64_t* mask_offset,
                           const unet_crop_desc* desc, int32_t n_crops, const int32_t* paste_start,
                           const unet_paste_desc* paste, int32_t n_pastes, int32_t out_h, int32_t out_w,
                           int32_t fill, int32_t ignore, uint8_t* dst_image, uint8_t* dst_mask, void* stream);

/* One fused step over a flat fp32 parameter arena: L2-coupled weight decay, bias correction,
 * gradient pre-scale (1/world_size under data parallelism). step is 1-based.  The betas are doubles so that 1 - beta is
 * formed in double before rounding to fp32, as torch.optim.Adam's `value=1 - beta2` is. */
int32_t unet_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                       float lr, double beta1, double beta2, float eps, float weight_decay,
                       float grad_scale, int32_t step, void* stream);

/* The optimiser step of get_optimizer's Adam / AdamW (src/train_utils.py:263-270) for ALL parameter tensors of a model in
 * ONE launch (the reference's torch.optim.Adam walks the 98 tensors): descs (DEVICE array) = one entry per tensor,
 * chunks (DEVICE array) = one entry per block: block b updates elements [first, first + unet_adam_chunk_elems()) of
 * tensor `tensor`.  Same arithmetic as unet_adam_step; decoupled != 0 = AdamW (p *= 1 - lr*wd instead of g += wd*p);
 * grad_scale folds the 1/world of data parallelism into the step. */
typedef struct unet_adam_desc {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
} unet_adam_desc;
typedef struct unet_adam_chunk {
  int32_t tensor;
  int32_t reserved;
  int64_t first;
} unet_adam_chunk;
int32_t unet_adam_chunk_elems(void);
int32_t unet_adam_multi(const unet_adam_desc* descs, const unet_adam_chunk* chunks, int32_t n_chunks, float lr, double beta1,
                        double beta2, float eps, float weight_decay, float grad_scale, int32_t step, int32_t decoupled,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNET_HIP_H_ */
