// The per-pixel rules of the segmentation kernels, stated once (segvis.hip, calibration.hip, tiles.hip, views.hip,
// defects.hip, segregions.hip, segeval.hip, segloss.hip; rankauc.hip takes `aligned`).
//   class_of      a label byte v has class v iff v < C; 0 and every value >= C are background.
//   conf_q        a confidence as 16.16 fixed point: (uint32) rint(clamp(v, 0, 1) * 65536), ties to even, NaN -> 0
//                 (fmaxf(NaN, 0) is 0).  The product is a scaling by a power of two, so it is exact whatever the
//                 contraction mode; integer sums of q are exact in any order.
//   argmax_conf   label = the FIRST maximum of the logits (strict >: torch.argmax), conf = softmax(z).max() stated as
//                 1 / sum_j expf(z_j - z_max), j in class order, all fp32; with SCALED the term is
//                 expf((z_j - z_max) * inv_t) and the label still comes from the raw logits (a rounding of z * inv_t can
//                 never move it).  (z_j - z_max) * 1.0f is z_j - z_max, so inv_t == 1 gives the unscaled bytes; the unscaled
//                 form compiles no multiply.  CM is the number of class slots the caller keeps in registers, C <= CM the
//                 class count; slots >= C are never read.
// For callers: the tests hold every user of argmax_conf to the same bits, and that needs every difference, product and
// sum rounded once.  The float arithmetic here takes the contraction mode of the including file, so every file that calls
// argmax_conf is built with -ffp-contract=off (its per-object line in the Makefile).
#pragma once
#include "common.h"

namespace segpx {

constexpr int MAXC = 8;                                // class slots of the segmentation head, loss, metrics and pictures

inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

__device__ __forceinline__ int class_of(uint8_t v, int C) { return v < C ? v : 0; }

__device__ __forceinline__ unsigned conf_q(float v) {
  return (unsigned)rintf(fminf(fmaxf(v, 0.0f), 1.0f) * 65536.0f);
}

template <bool SCALED = false, int CM>
__device__ __forceinline__ int argmax_conf(const float (&z)[CM], int C, float& conf, float inv_t = 1.0f) {
  float best = z[0];
  int arg = 0;
#pragma unroll
  for (int c = 1; c < CM; ++c)
    if (c < C && z[c] > best) { best = z[c]; arg = c; }
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < CM; ++c) {
    if (c < C) {
      if constexpr (SCALED) s += expf((z[c] - best) * inv_t);
      else s += expf(z[c] - best);
    }
  }
  conf = 1.0f / s;
  return arg;
}

}  // namespace segpx
