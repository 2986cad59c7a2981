// Smoothing of anomaly maps for the MVTec evaluation (test.py --map_sigma / --image_score map_max), one kernel per batch.
//
// The reference ranks the raw map and scores an image by its mean reconstruction error (src/test.py:66-133); the
// published MVTec AD protocols smooth the map (a Gaussian of sigma 4 in PaDiM / PatchCore) and score an image by the
// map's peak.  This file is that step on the device; tests/_smooth_ref.py restates it in float64.
//
//   dst     the separable correlation of src along W, then along H, with the symmetric kernel taps[|k|], k = -r .. r
//   border  scipy's `reflect` (d c b a | a b c d | d c b a), folded as often as needed: index i -> j = i mod 2L, then
//           2L - 1 - j if j >= L.  Sides shorter than the radius (down to 1) fold several times.
//   sum     fp32: acc = taps[0] * x[0], then acc = fma(taps[k], x[-k] + x[+k], acc) for k = 1 .. r, in both passes
//   max     image_max[i] = the largest element written to plane i, NaN if any is NaN
//
// A block owns a 32 x 64 tile of one plane.  It stages the tile and its halo ((32 + 2r) rows of 64 + 2 * pad4(r)
// columns, already folded) in LDS, runs the W pass in place -- a thread reads the window of four neighbouring outputs
// with 16-byte LDS reads into registers, a wave owns four whole staged rows: all of its reads come before its stores in
// program order, and no other wave touches those rows in that phase -- and the H pass from there, four columns per
// thread with 16-byte LDS reads.  The kernel is compiled once per pad4(r), so the tap loops unroll.  The row stride is
// 64 or 128 floats (32 KB at r <= 16, 48 KB at r = 32: three to four blocks per CU), a multiple of the 64 banks, so the
// four 16-lane groups of a 16-byte read, which fall on different rows, never meet on a bank.  Global accesses are 16
// bytes wide when w % 4 == 0 and src / dst are 16-byte aligned (every plane then starts aligned); groups of four that
// cross a border, and every other case, go element by element.
//
// The maximum travels as an order-preserving integer key (NaN on top) through the wave and the block, and reaches
// image_max with one integer atomic per tile: atomicMax on the bits as int for a value with the sign bit clear,
// atomicMin on the bits as unsigned for one with it set, so the word always holds the float itself.  The launcher
// fills image_max with 0xFF bytes (below everything under both orders) on the stream ahead of the kernel.  Integer
// atomics commute: the result does not depend on the order of arrival.
#include "common.h"

#include <cmath>

namespace {

constexpr int SM_TH = 32, SM_TW = 64;
constexpr int SM_THREADS = 256;
constexpr int SM_MAX_BLOCKS = 2048;        // 256 CUs x 8 blocks; the rest of a larger batch comes through the stride loop
constexpr int SM_KEY_NAN = 0x7fffffff;
constexpr int SM_KEY_NONE = (int)0x80000000u;

struct SmoothTaps {
  float w[UNET_SMOOTH_MAX_RADIUS + 1];
};

__host__ __device__ inline int pad4(int r) { return (r + 3) & ~3; }
__host__ __device__ inline int row_stride(int r) { return (SM_TW + 2 * pad4(r) + 63) & ~63; }

// scipy's reflect: (d c b a | a b c d | d c b a)
// (i lies within a tile and a halo of [0, L): a 64-bit sum of ints, between -2^31 and 2^32 - 1)
__device__ __forceinline__ int fold(long long i, int L) {
  if ((unsigned long long)i < (unsigned long long)L) return (int)i;
  if (i < 0) i = -1 - i;                        // the border is symmetric about -1/2
  unsigned u = (unsigned)i;
  const unsigned l = (unsigned)L, p = 2u * l;   // L <= 2^31 - 1: p fits
  if (u >= p) u %= p;                           // (only a side shorter than the halo folds more than once)
  return (int)(u >= l ? p - 1u - u : u);
}

// monotone in the float order, -0.0 below +0.0, every NaN on top
__device__ __forceinline__ int max_key(float v) {
  const int b = __float_as_int(v);
  if (v != v) return SM_KEY_NAN;
  return b >= 0 ? b : b ^ 0x7fffffff;
}

// VEC: 16-byte global accesses (w % 4 == 0, src and dst 16-byte aligned).  RP = pad4(R): the loops over the taps are
// unrolled to it, so the taps sit in scalar registers and the window of the W pass in vector registers; the last three
// steps ask whether they are within R (a tap is never padded with zero: 0 * inf would be NaN).
template <bool VEC, int RP>
__global__ __launch_bounds__(SM_THREADS) void smooth_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                            long long tiles, int tiles_y, int tiles_x, int H, int W,
                                                            SmoothTaps taps, int R, int* __restrict__ image_max) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int SW = SM_TW + 2 * RP, SS = (SW + 63) & ~63, G = SW / 4;
  const int SH = SM_TH + 2 * R;
  int* wave_max = reinterpret_cast<int*>(lds + SH * SS);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float w0 = taps.w[0];

  for (unsigned tile = blockIdx.x; tile < (unsigned)tiles; tile += gridDim.x) {      // (tiles <= n * h * w < 2^31)
    const unsigned per = (unsigned)(tiles_y * tiles_x);
    const int img = (int)(tile / per), rem = (int)(tile - (unsigned)img * per);
    const int y0 = rem / tiles_x * SM_TH, x0 = rem % tiles_x * SM_TW;
    const float* plane = src + (long long)img * H * W;

    // ---- stage rows y0 - R .. y0 + TH + R, columns x0 - RP .. x0 + TW + RP, folded
    if (VEC) {
      for (int item = tid; item < SH * G; item += SM_THREADS) {
        const int sy = item / G, g = item - sy * G;
        const float* row = plane + (long long)fold((long long)y0 - R + sy, H) * W;
        const long long gx = (long long)x0 - RP + 4 * g;
        f32x4 v;
        if (gx >= 0 && gx + 3 < W) {
          v = *reinterpret_cast<const f32x4*>(row + gx);
        } else {
          v[0] = row[fold(gx, W)]; v[1] = row[fold(gx + 1, W)]; v[2] = row[fold(gx + 2, W)]; v[3] = row[fold(gx + 3, W)];
        }
        *reinterpret_cast<f32x4*>(lds + sy * SS + 4 * g) = v;
      }
    } else {
      for (int item = tid; item < SH * SW; item += SM_THREADS) {
        const int sy = item / SW, sx = item - sy * SW;
        lds[sy * SS + sx] = plane[(long long)fold((long long)y0 - R + sy, H) * W + fold((long long)x0 - RP + sx, W)];
      }
    }
    __syncthreads();

    // ---- W pass, in place: staged row sy, columns RP + 4q .. + 3 -> columns 4q .. + 3.  16 threads per row, so a wave
    // owns four whole rows: it reads their windows (RP / 2 + 1 16-byte reads each) before it stores, and no other wave
    // touches those rows in this phase.
    for (int item = tid; item < SH * 16; item += SM_THREADS) {
      float* c = lds + (item >> 4) * SS + 4 * (item & 15);
      float win[2 * RP + 4];
#pragma unroll
      for (int m = 0; m <= RP / 2; ++m) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(c + 4 * m);
        win[4 * m] = v[0]; win[4 * m + 1] = v[1]; win[4 * m + 2] = v[2]; win[4 * m + 3] = v[3];
      }
      f32x4 acc;
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = w0 * win[RP + i];
#pragma unroll
      for (int k = 1; k <= RP; ++k)
        if (k <= RP - 4 || k <= R) {
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[i] = fmaf(taps.w[k], win[RP + i - k] + win[RP + i + k], acc[i]);
        }
      *reinterpret_cast<f32x4*>(c) = acc;
    }
    __syncthreads();

    // ---- H pass: 4 columns per thread, 16 rows per sweep; store and keep the largest key
    int key = SM_KEY_NONE;
    const int qx = 4 * (tid & 15);
    for (int ry = tid >> 4; ry < SM_TH; ry += SM_THREADS / 16) {
      const float* c = lds + (ry + R) * SS + qx;
      f32x4 acc = w0 * *reinterpret_cast<const f32x4*>(c);
#pragma unroll
      for (int k = 1; k <= RP; ++k)
        if (k <= RP - 4 || k <= R) {
          const f32x4 pair = *reinterpret_cast<const f32x4*>(c - k * SS) + *reinterpret_cast<const f32x4*>(c + k * SS);
          const float wk = taps.w[k];
          acc[0] = fmaf(wk, pair[0], acc[0]); acc[1] = fmaf(wk, pair[1], acc[1]);
          acc[2] = fmaf(wk, pair[2], acc[2]); acc[3] = fmaf(wk, pair[3], acc[3]);
        }
      if (ry < H - y0 && qx < W - x0) {
        float* out = dst + ((long long)img * H + y0 + ry) * W + x0 + qx;
        if (VEC) {                                      // (w % 4 == 0: a group that starts inside the row ends inside it)
          *reinterpret_cast<f32x4*>(out) = acc;
#pragma unroll
          for (int j = 0; j < 4; ++j) key = max(key, max_key(acc[j]));
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (qx + j < W - x0) {
              out[j] = acc[j];
              key = max(key, max_key(acc[j]));
            }
        }
      }
    }
    if (image_max) {
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) key = max(key, __shfl_xor(key, d, 64));
      if (lane == 0) wave_max[wave] = key;
    }
    __syncthreads();            // (also: the next tile's staging overwrites what the H pass read)
    if (image_max && tid == 0) {
      key = max(max(wave_max[0], wave_max[1]), max(wave_max[2], wave_max[3]));
      if (key != SM_KEY_NONE) {
        const int bits = key == SM_KEY_NAN ? 0x7fc00000 : key >= 0 ? key : key ^ 0x7fffffff;
        if (bits >= 0)
          atomicMax(image_max + img, bits);
        else
          atomicMin(reinterpret_cast<unsigned*>(image_max + img), (unsigned)bits);
      }
    }
  }
}

}  // namespace

extern "C" int32_t unet_smooth_maps(const float* src, float* dst, int64_t n, int32_t h, int32_t w, const float* taps,
                                    int32_t radius, float* image_max, void* stream) {
  UNET_REQUIRE(src && dst && taps, UNET_ERR_BAD_ARG, "unet_smooth_maps: null pointer (src %p, dst %p, taps %p)",
               (const void*)src, (const void*)dst, (const void*)taps);
  UNET_REQUIRE(n >= 0 && h >= 0 && w >= 0, UNET_ERR_BAD_ARG, "unet_smooth_maps: batch %lld x %d x %d", (long long)n, h, w);
  UNET_REQUIRE(radius >= 0, UNET_ERR_BAD_ARG, "unet_smooth_maps: radius %d", radius);
  UNET_REQUIRE(radius <= UNET_SMOOTH_MAX_RADIUS, UNET_ERR_UNSUPPORTED, "unet_smooth_maps: radius %d (at most %d)", radius,
               UNET_SMOOTH_MAX_RADIUS);
  SmoothTaps t = {};
  for (int k = 0; k <= radius; ++k) {
    UNET_REQUIRE(std::isfinite(taps[k]), UNET_ERR_BAD_ARG, "unet_smooth_maps: tap %d is %f", k, (double)taps[k]);
    t.w[k] = taps[k];
  }
  const int64_t hw = (int64_t)h * w;
  UNET_REQUIRE(hw == 0 || n <= INT32_MAX / hw, UNET_ERR_UNSUPPORTED,
               "unet_smooth_maps: %lld x %d x %d elements (at most 2^31 - 1)", (long long)n, h, w);
  const int64_t total = n * hw;
  const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst, bytes = (uintptr_t)total * 4;
  UNET_REQUIRE(a != b && (total == 0 || (a + bytes <= b || b + bytes <= a)), UNET_ERR_BAD_ARG,
               "unet_smooth_maps: src %p and dst %p overlap (%lld bytes each)", (const void*)src, (const void*)dst,
               (long long)bytes);
  if (total == 0) return UNET_OK;

  hipStream_t s = (hipStream_t)stream;
  const int tiles_y = (int)cdiv64(h, SM_TH), tiles_x = (int)cdiv64(w, SM_TW);
  const long long tiles = (long long)n * tiles_y * tiles_x;
  const int blocks = (int)(tiles < SM_MAX_BLOCKS ? tiles : SM_MAX_BLOCKS);
  const size_t lds_bytes = (size_t)(SM_TH + 2 * radius) * row_stride(radius) * 4 + 16;
  const bool vec = w % 4 == 0 && ((a | b) & 15) == 0;
  ProfScope prof(UNET_K_OTHER, 2.0 * (3 * radius + 1) * (double)total, s, vec ? "smooth_kernel<vec>" : "smooth_kernel<scalar>",
                 8.0 * (double)total + (image_max ? 4.0 * (double)n : 0.0));
  if (image_max && hipMemsetAsync(image_max, 0xff, (size_t)n * 4, s) != hipSuccess)
    return unet_check_launch("unet_smooth_maps: image_max fill");
  int* mx = reinterpret_cast<int*>(image_max);
#define SMOOTH_LAUNCH(V, RP_)                                                                                            \
  hipLaunchKernelGGL((smooth_kernel<V, RP_>), dim3(blocks), dim3(SM_THREADS), lds_bytes, s, src, dst, tiles, tiles_y, \
                     tiles_x, h, w, t, radius, mx)
#define SMOOTH_CASE(RP_)                \
  case RP_:                             \
    if (vec)                            \
      SMOOTH_LAUNCH(true, RP_);         \
    else                                \
      SMOOTH_LAUNCH(false, RP_);        \
    break;
  switch (pad4(radius)) {
    SMOOTH_CASE(0) SMOOTH_CASE(4) SMOOTH_CASE(8) SMOOTH_CASE(12) SMOOTH_CASE(16) SMOOTH_CASE(20) SMOOTH_CASE(24)
    SMOOTH_CASE(28) SMOOTH_CASE(32)
    default:
      unet_set_error("unet_smooth_maps: radius %d", radius);          // (refused above)
      return UNET_ERR_UNSUPPORTED;
  }
#undef SMOOTH_CASE
#undef SMOOTH_LAUNCH
  return unet_check_launch(vec ? "smooth_kernel<vec>" : "smooth_kernel<scalar>");
}
