// What the two sheet renderers share (render.hip: the MVTec evaluation sheet; segvis.hip: the Gear / KolektorSDD
// prediction sheet).  A sheet is packed uint8 RGB, panels of H x W pixels with gutters of 255 between them.  A thread
// produces RUN = 4 consecutive pixels of one sheet row = 12 bytes = 3 dwords, stored as dwords where the run is whole and
// its address dword-aligned, else byte by byte.  A pixel travels as one uint32: red in the lowest byte, 0 in the highest.
// The float steps (denormalise, scale to a byte) restate matplotlib's float32 arithmetic, every product and sum rounded
// once: they take the contraction mode of the including file, and both renderers are built with -ffp-contract=off.
#pragma once
#include "common.h"

namespace sheet {

constexpr int RUN = 4;                                 // pixels per thread
constexpr uint32_t WHITE = 0x00ffffffu;

// clamp to [0, 1] (NaN -> 0), then the truncating byte of matplotlib's (x * 255).astype(uint8) on float32
__device__ __forceinline__ uint32_t unit_byte(float v) {
  if (!(v > 0.f)) v = 0.f;
  if (v > 1.f) v = 1.f;
  return (uint32_t)(v * 255.0f);
}
// a normalised input pixel back to [0, 1]: v * std[c], then + mean[c]
__device__ __forceinline__ void denormalise(const float (&mean)[3], const float (&std)[3], float& r, float& g, float& b) {
  r = r * std[0]; r = r + mean[0];
  g = g * std[1]; g = g + mean[1];
  b = b * std[2]; b = b + mean[2];
}
// (a8 * top + (255 - a8) * img + 127) / 255 in integers per channel
__device__ __forceinline__ uint32_t blend(uint32_t top, uint32_t img, uint32_t a8) {
  uint32_t out = 0;
#pragma unroll
  for (int s = 0; s < 24; s += 8)
    out |= ((a8 * ((top >> s) & 255u) + (255u - a8) * ((img >> s) & 255u) + 127u) / 255u) << s;
  return out;
}

// thread t packs entry `first + t` of a byte table of [3]-byte entries into tab[t]: a block of 256 threads stages a
// 256-entry table; a barrier comes before the first use
__device__ __forceinline__ void stage_table(uint32_t* tab, const uint8_t* table, int first = 0) {
  const uint8_t* e = table + (first + threadIdx.x) * 3;
  tab[threadIdx.x] = (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16);
}

// The run walk: the kernels stride the grid over the runs of the sheet, rw = cdiv(SW, RUN) runs to a row of SW pixels; a
// run is at least 3 bytes of a sheet of fewer than 2^31, so run indices are 32-bit.  Run t starts at pixel col0 of sheet
// row `row` and has cnt >= 1 pixels inside the row.
struct Run { int row, col0, cnt; };
__device__ __forceinline__ Run run_at(uint32_t t, uint32_t rw, int SW) {
  const int col0 = (int)(t % rw) * RUN;
  return Run{(int)(t / rw), col0, min(RUN, SW - col0)};
}

// The run store (three dwords where the run is whole and its address dword-aligned, else byte by byte) stays written
// out in the two kernels: as a function it changed their device code (profiles/shared_bodies.txt).

}  // namespace sheet
