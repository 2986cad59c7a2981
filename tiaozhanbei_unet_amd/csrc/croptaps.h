// The sample of one output pixel of an affine crop: where its taps lie and how they are weighed (the rule of
// unet_affine_crop_u8, include/unet_hip.h).  Shared by crops.hip and paste.hip, so both cut the same bytes.
#pragma once
#include <cstdint>

namespace {

// where the taps of one output pixel lie (element offsets of the pixel's first channel) and their weights
struct Taps {
  bool inside;
  long long o00, o01, o10, o11;                        // nearest: o00 alone
  int fx, fy;
};

// the four bilinear taps around (u, v) (16.16, half-pixel terms included), each clamped into the image, and fx, fy
__device__ __forceinline__ void bilinear_taps(Taps& t, long long u, long long v, int h, int w, int c) {
  const long long ub = u - 32768, vb = v - 32768;
  long long x0 = ub >> 16, y0 = vb >> 16;
  long long x1 = x0 + 1, y1 = y0 + 1;
  t.fx = (int)((ub & 0xFFFF) >> 8);
  t.fy = (int)((vb & 0xFFFF) >> 8);
  const long long wm = w - 1, hm = h - 1;
  x0 = x0 < 0 ? 0 : (x0 > wm ? wm : x0);
  x1 = x1 < 0 ? 0 : (x1 > wm ? wm : x1);
  y0 = y0 < 0 ? 0 : (y0 > hm ? hm : y0);
  y1 = y1 < 0 ? 0 : (y1 > hm ? hm : y1);
  t.o00 = (y0 * w + x0) * c; t.o01 = (y0 * w + x1) * c;
  t.o10 = (y1 * w + x0) * c; t.o11 = (y1 * w + x1) * c;
}

template <int MODE>
__device__ __forceinline__ Taps taps_of(long long u, long long v, int h, int w, int c) {
  Taps t;
  const long long nx = u >> 16, ny = v >> 16;
  t.inside = nx >= 0 && nx < w && ny >= 0 && ny < h;
  t.o00 = t.o01 = t.o10 = t.o11 = 0;
  t.fx = t.fy = 0;
  if (!t.inside) return t;
  if constexpr (MODE == 0) {
    t.o00 = (ny * w + nx) * c;
  } else {
    bilinear_taps(t, u, v, h, w, c);
  }
  return t;
}

template <int MODE>
__device__ __forceinline__ unsigned sample(const uint8_t* __restrict__ img, const Taps& t, int ch, int fill) {
  if (!t.inside) return (unsigned)fill;
  if constexpr (MODE == 0) {
    return img[t.o00 + ch];
  } else {
    const int p00 = img[t.o00 + ch], p01 = img[t.o01 + ch], p10 = img[t.o10 + ch], p11 = img[t.o11 + ch];
    const int top = (256 - t.fx) * p00 + t.fx * p01, bot = (256 - t.fx) * p10 + t.fx * p11;
    return (unsigned)(((256 - t.fy) * top + t.fy * bot + 32768) >> 16);
  }
}

}  // namespace
