// Shared device/host helpers for libunet_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/unet_hip.h"

typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

#define WAVE 64

// ---- host side status handling ---------------------------------------------------------
void unet_set_error(const char* fmt, ...);
int32_t unet_check_launch(const char* what);

#define UNET_REQUIRE(cond, code, ...)  \
  do {                                 \
    if (!(cond)) {                     \
      unet_set_error(__VA_ARGS__);     \
      return (code);                   \
    }                                  \
  } while (0)

// CUs the persistent (one-block-per-CU, statically partitioned) kernels may count on: the device's multiprocessor count
// minus unet_set_reserved_cus() (a data-parallel run leaves a few CUs to the RCCL all-reduce kernels that overlap the
// backward pass -- with all 256 claimed, a conv launch would wait for the CUs a collective holds and a static partition
// then takes up to twice as long), rounded down to a multiple of 8 (XCDs), at least 8
int unet_cu_budget();
// opt a kernel in to `bytes` of dynamic LDS -- once per (device, kernel), cheap afterwards
void unet_set_max_lds(const void* kernel, int bytes);

// ---- per-class event timing (prof.cpp) ---------------------------------------------------
void unet_prof_begin(int kclass, hipStream_t s);
void unet_prof_end(int kclass, double flops, hipStream_t s, const char* kernel, double bytes);
struct ProfScope {
  int k; double f; hipStream_t s; const char* name;      // name: static string naming the (dominant) kernel of the bracket
  double bytes;                                          // algorithmic bytes of the launch: inputs + weights + outputs, each once
  ProfScope(int kclass, double flops, hipStream_t st, const char* kernel = nullptr, double alg_bytes = 0.0)
      : k(kclass), f(flops), s(st), name(kernel), bytes(alg_bytes) {
    unet_prof_begin(k, s);
  }
  ~ProfScope() { unet_prof_end(k, f, s, name, bytes); }
};

// the deep transposed convolutions as one LDS-DMA GEMM (convt_gemm.hip); mode 0 forward, 1 data gradient
bool unet_internal_convt_gemm_ok(int mode, int dtype, int n, int h, int w, int c_in, int c_out);
int32_t unet_internal_convt_gemm(int mode, int n, int h, int w, const void* a, const void* w_packed, const float* bias,
                                 void* out, int c_in, int c_out, hipStream_t s);

// deterministic per-channel sum of x[pixels][C] (bn.hip); ws is scratch
int32_t unet_internal_colsum(int dtype, const void* x, int64_t pixels, int C, float* out, float* ws,
                              size_t ws_bytes, hipStream_t s);

// BatchNorm partial sums [parts][2][C] of y[pixels][C] by one streaming pass (bn.hip); parts <= 1024
int32_t unet_internal_bn_partials(int dtype, const void* y, int64_t pixels, int C, float* part, int* n_parts,
                                  hipStream_t s);

// ---- element traits ----------------------------------------------------------------------
template <typename T> struct ET;
template <> struct ET<float> {
  static constexpr int ES = 4;          // bytes per element
  static constexpr int PIECE = 4;       // elements per 16-byte piece
  static constexpr int KGC = 8;         // channels per 32-byte k-group
  __device__ static inline float to_f(float v) { return v; }
  __device__ static inline float from_f(float v) { return v; }
};
template <> struct ET<bf16_t> {
  static constexpr int ES = 2;
  static constexpr int PIECE = 8;
  static constexpr int KGC = 16;
  __device__ static inline float to_f(bf16_t v) { return (float)v; }
  __device__ static inline bf16_t from_f(float v) { return (bf16_t)v; }
};

// 16-byte vector load/store of PIECE elements, converted to/from fp32
template <typename T> struct Vec;
template <> struct Vec<float> {
  static constexpr int N = 4;
  __device__ static inline void load(const float* p, float (&o)[4]) {
    f32x4 v = *reinterpret_cast<const f32x4*>(p);
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
  }
  __device__ static inline void store(float* p, const float (&o)[4]) {
    f32x4 v = {o[0], o[1], o[2], o[3]};
    *reinterpret_cast<f32x4*>(p) = v;
  }
};
template <> struct Vec<bf16_t> {
  static constexpr int N = 8;
  __device__ static inline void load(const bf16_t* p, float (&o)[8]) {
    bf16x8 v = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = (float)v[i];
  }
  __device__ static inline void store(bf16_t* p, const float (&o)[8]) {
    bf16x8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (bf16_t)o[i];
    *reinterpret_cast<bf16x8*>(p) = v;
  }
};

static inline bool dtype_known(int dtype) { return dtype == UNET_F32 || dtype == UNET_BF16; }
// The one way from a runtime dtype to an element type: f(bf16_t{}) or f(float{}), and the callee writes
// `using T = decltype(tag);`.  Any other dtype is refused here, before f -- so before anything f times or launches.
template <typename F>
int32_t with_dtype(const char* who, int dtype, F&& f) {
  if (dtype == UNET_BF16) return f(bf16_t{});
  if (dtype == UNET_F32) return f(float{});
  unet_set_error("%s: dtype %d", who, dtype);
  return UNET_ERR_BAD_ARG;
}

__host__ __device__ static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
__host__ __device__ static inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- scores as sort keys (rankauc.hip, render.hip) ------------------------------------------
// order-preserving key of a finite float: -0.0 == +0.0 first, then sign-magnitude -> unsigned order
__device__ __forceinline__ uint32_t score_key(float x) {
  uint32_t u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float score_of_key(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ bool finite_score(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// ---- segment map of a two-source (skip | up-sampled) convolution input with a narrow first source (widths.hip) ------
// Packed column q of the padded input -> column of the parameter's input axis, or -1 (a zero column).  split = logical
// channels of source 0; source 1 starts at pad64(split).  split == 0: contiguous, the columns >= c are zero.
__host__ __device__ static inline int unet_seg_col(int q, int split, int c) {
  if (split > 0 && q >= split) {
    const int p0 = (split + 63) / 64 * 64;
    if (q < p0) return -1;
    q = q - p0 + split;
  }
  return q < c ? q : -1;
}

// element i of a 3x3 conv weight packed (UNET_PACK_CONV_FWD [9][rows][k] / UNET_PACK_CONV_DGRAD [9 flipped][rows][k])
// through the segment map `split` of its input-channel axis; scale (may be NULL): BatchNorm fold per output channel
__device__ static inline float unet_pack_seg_value(const float* __restrict__ w, int Co, int Ci, int rows, int K, int mode,
                                                   int split, long long i, const float* __restrict__ scale) {
  const int b = (int)(i % K);
  const long long t = i / K;
  const int a = (int)(t % rows), tap = (int)(t / rows);
  if (mode == UNET_PACK_CONV_FWD) {                // a = co, b = packed input column
    const int ci = unet_seg_col(b, split, Ci);
    return (a < Co && ci >= 0) ? w[((long long)a * Ci + ci) * 9 + tap] * (scale ? scale[a] : 1.f) : 0.f;
  }
  const int ci = unet_seg_col(a, split, Ci);       // a = packed input row, b = co
  return (b < Co && ci >= 0) ? w[((long long)b * Ci + ci) * 9 + (8 - tap)] : 0.f;
}
