// What the convolution kernel families (igemm.hip, conv3.hip, conv3_pdma.hip, conv3_ws.hip, convt_ws.hip) and their
// entry points (conv_api.hip) share: parameter structs, the register-staged tile, the DPP row reduction, the launchers.
#pragma once
#include "common.h"
#include "stamps.h"

struct DView { const char* p; int C, H, W, oy, ox; };
struct DViewW { char* p; int C, H, W, oy, ox; };

struct IgemmParams {
  DView src[2];
  DViewW dst[2];
  int N, H, W;      // GEMM pixel grid (the logical frame)
  int Ctot;         // input channels per (gather) tap = src[0].C + src[1].C
  int Cout;         // GEMM rows
  int wK;           // weight row length in elements
  const char* w;
  const float* bias;
  int dst_split;
  int accumulate;
  int relu;         // != 0: max(., 0) after the bias (inference with BatchNorm folded into weights + bias)
  int imul, gtaps;  // input position = frame*imul + gather tap (convT dgrad: 2, 4)
  int omul, nZ;     // output position = frame*omul + z tap     (convT fwd:   2, 4)
  int zdiv;         // > 0: GEMM row = z*zdiv + co (convT fwd as one GEMM with 4*Cout rows)
  float* stats;     // != NULL: per-block BatchNorm partials [part][2][Cout] written by the epilogue
  int tilesX, tilesY, nCo;
  // data gradient fused with the ReLU mask + BatchNorm-backward sums of the layer that PRODUCED this convolution's
  // input (kernels instantiated with BNBWD): bn_y = that layer's raw conv output [N][H][W][Cout] (same geometry as
  // dst[0]), bn_scale / bn_shift / bn_mean = its forward coefficients.  The epilogue stores dz = dx * [fma(y, scale,
  // shift) > 0] and the partial sums (sum dz, sum dz * (y - mean)) go where the forward statistics would (stats).
  const char* bn_y;
  const float* bn_scale;
  const float* bn_shift;
  const float* bn_mean;
  int co_il;        // conv3_pdma: channel tiles interleaved per pixel tile in the work order (1, 2 or 4; see pdma_item)
  int pdma_stagger; // conv3_pdma (lock-step): DMA issues of a SIMD's two waves at opposite ends of a tap; always 1 (a
                    // run-time value on purpose: as a constant, hipcc gives conv3_pdma64x2_kernel 181 instead of 177 VGPRs)
  int pdma_dense;   // conv3_pdma: every destination view covers the frame at offset 0 (scalar output addressing)
  int pdma_dense_src; // conv3_pdma: every source view covers the frame at offset 0, one channel stride (scalar patch addressing)
#ifdef PDMA_STAMPS
  StampSink stamps;   // diagnostic build only, last: where conv3_pdma_body / conv3_ws16_kernel write their stamp records
#endif
};

struct ConvTParams {
  const char* x; char* y; const char* w; const float* bias;
  int N, H, W, Cout;      // input spatial dims; output is [N][2H][2W][Cout]
  int tiles, tiles_per_block;
  // data gradient fused with the ReLU mask and the BatchNorm-backward sums of the layer that produced the transposed
  // convolution's input (convt_dgrad_ws_kernel<COUT, true>): that layer's raw conv output, its coefficients, the
  // partial sums [blocks][2][CIN]
  const char* bn_y; const float* bn_scale; const float* bn_shift; const float* bn_mean; float* stats;
};

// output tile of the register-staged kernels (igemm.hip, conv3.hip) and of unet_conv3x3_stats_max_parts
constexpr int TH = 8, TW = 16, NPIX = TH * TW;

template <typename View>   // the view covers the frame at offset 0
inline bool covers_frame(const View& v, const IgemmParams& P) { return !v.oy && !v.ox && v.H == P.H && v.W == P.W; }

// sum over the 16 lanes of a DPP row, for N >= 3 independent values at once: v_add_f32 with a DPP source operand, one
// instruction per value and step (quad xor 1, quad xor 2, half-row mirror, row mirror; fixed order -> deterministic).
// Through __builtin_amdgcn_update_dpp hipcc emitted v_mov_b32 (old = 0) + v_mov_b32_dpp + half a v_pk_add_f32 per step
// (its packed-add vectoriser defeats the DPP combine): 2.4x the instructions.  Step-major order + `asm volatile` (kept in
// source order) puts N - 1 >= 2 instructions between the VALU write of a value and the DPP read of it -- the wait states
// hipcc does not pad inside asm; one s_nop covers the producers of the inputs.  dst = dpp(src) + src: the same sums, bit
// for bit.
template <int N>
__device__ __forceinline__ void row16_sum_n(float (&v)[N]) {
  static_assert(N >= 3, "hazard distance");
  asm volatile("s_nop 1");
#pragma unroll
  for (int i = 0; i < N; ++i)
    asm volatile("v_add_f32_dpp %0, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "=v"(v[i]) : "0"(v[i]));
#pragma unroll
  for (int i = 0; i < N; ++i)
    asm volatile("v_add_f32_dpp %0, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf" : "=v"(v[i]) : "0"(v[i]));
#pragma unroll
  for (int i = 0; i < N; ++i)
    asm volatile("v_add_f32_dpp %0, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xf" : "=v"(v[i]) : "0"(v[i]));
#pragma unroll
  for (int i = 0; i < N; ++i)
    asm volatile("v_add_f32_dpp %0, %1, %1 row_mirror row_mask:0xf bank_mask:0xf" : "=v"(v[i]) : "0"(v[i]));
}

// ---- the launchers of the families, called by dispatch<> and the entry points (conv_api.hip) -----------------------
// igemm.hip, T = bf16_t / float, TAPS = 9 / 1: igemm_kernel<T, TAPS, big ? 128 : 64, k4 ? 4 : 1>
template <typename T, int TAPS>
int32_t unet_internal_igemm(const IgemmParams& P, bool big, bool k4, int kclass, hipStream_t s);
// conv3.hip, T = bf16_t / float: conv3_kernel / conv3m16_kernel<T, big ? 128 : 64, k4 ? 4 : 1>
template <typename T>
int32_t unet_internal_conv3(const IgemmParams& P, bool big, bool k4, int kclass, hipStream_t s, int* stat_parts);
// conv3_pdma.hip (128-channel tiles where P.Cout is a multiple of 128, 64-channel tiles otherwise), conv3_ws.hip
int32_t unet_internal_conv3_pdma(const IgemmParams& P, int kclass, hipStream_t s, int* stat_parts);
int32_t unet_internal_conv3_ws(IgemmParams P, int kclass, hipStream_t s, int* stat_parts);
// convt_ws.hip: c_in = 128 / 256 (forward), c_out = 64 / 128 (data gradient)
int32_t unet_internal_convt_ws(int c_in, ConvTParams P, hipStream_t s);
int32_t unet_internal_convt_dgrad_ws(int c_out, ConvTParams P, hipStream_t s, int* n_parts = nullptr);
