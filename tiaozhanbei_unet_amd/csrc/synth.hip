// Synthetic anomalies for the MVTec trainer (train.py --synthetic_anomalies), one launch per batch.
//
// The reference has nothing like this (its train split is train/good only: every training mask is zero and the
// reconstruction target is the network's own input), so there is no code to restate.  The DEFINITION below is this
// project's own and tests/_synth_ref.py restates it independently in numpy; the kernel equals that restatement bit for
// bit (IEEE single precision, every product and sum rounded once, on both sides).
//
//   noise   2-D gradient (Perlin) noise at pixel centres.  Along an axis of length n with L cells (L = 1, 2, .. 64) pixel p
//           lies in cell i = (2pL + L) / (2n) at fraction t = ((2pL + L) % (2n)) / (2n), rounded to fp32, and
//           fade(t) = t*t*t*(t*(t*6 - 15) + 10) in fp32.  i, t and fade come from HOST tables (augment.py builds them once
//           per axis length for the seven lattice sizes): the kernel reads three values per axis instead of dividing.
//   lattice the gradient at lattice point (iy, ix) is entry hash(seed, iy, ix) & 255 of a table of 256 unit vectors
//           (cos 2 pi k / 256, sin 2 pi k / 256), computed in double by the host and rounded to fp32, with
//               h  = seed + iy * 0x9E3779B1 + ix * 0x85EBCA77              (all in uint32, wrapping)
//               h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16      (murmur3's finaliser)
//   value   with (gx, gy) the gradient of a corner and (dx, dy) the offset from it: dot = gx*dx + gy*dy, dx in {tx, tx - 1},
//           dy in {ty, ty - 1};  lerp(a, b, f) = a + f*(b - a);  top = lerp(d00, d10, fade x), bottom = lerp(d01, d11,
//           fade x) (d<y><x>), noise = lerp(top, bottom, fade y) * fp32(sqrt 2)  -- roughly [-1, 1]
//   mask    m = apply && noise > threshold;  mask out = max(mask in, m)   (m alone without a mask input)
//   blend   where m: out[c] = beta * x[c] + one_minus_beta * donor[perm(c)], the donor pixel being image `src` of the same
//           batch at ((y + shift_y) mod H, (x + shift_x) mod W); elsewhere out = x, bit for bit.
//
// A pure stream: 3 planes in, about 3 scattered donor reads where the mask is set, 3 planes + 1 mask out.  The noise is
// computed once per pixel for the three channels, the four corner gradients once per run of pixels in the same cell.  When
// the plane size is a multiple of 4 every plane of every image starts 16-byte aligned and a thread moves 4 consecutive
// pixels of the flat plane (which may cross a row end) with 16-byte accesses; other sizes take one pixel per thread.
#include "common.h"

// every product and every sum rounds once (the Makefile passes -ffp-contract=off for this file as well)
#pragma clang fp contract(off)

namespace {

constexpr int SY_THREADS = 256;
constexpr int SY_MAX_BLOCKS = 2048;        // 256 CUs x 8 blocks; the rest of a larger batch comes through the stride loop

__device__ __forceinline__ uint32_t lattice_hash(uint32_t seed, uint32_t iy, uint32_t ix) {
  uint32_t h = seed + iy * 0x9E3779B1u + ix * 0x85EBCA77u;
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

__device__ __forceinline__ float lerp1(float a, float b, float f) { return a + f * (b - a); }

__device__ __forceinline__ bool pow2_upto64(int v) { return v >= 1 && v <= 64 && (v & (v - 1)) == 0; }

// V = 4: 16-byte accesses, needs H * W % 4 == 0.  V = 1: any size.
template <int V>
__global__ __launch_bounds__(SY_THREADS) void synth_kernel(const float* __restrict__ img, const float* __restrict__ mask_in,
                                                           float* __restrict__ out, float* __restrict__ mask_out, int N,
                                                           int H, int W, const unet_synth_desc* __restrict__ desc,
                                                           const int* __restrict__ ycell, const float* __restrict__ ytf,
                                                           const int* __restrict__ xcell, const float* __restrict__ xtf,
                                                           const float* __restrict__ grad) {
  __shared__ float gtab[256][2];
  gtab[threadIdx.x][0] = grad[2 * threadIdx.x];
  gtab[threadIdx.x][1] = grad[2 * threadIdx.x + 1];
  __syncthreads();

  const unsigned HW = (unsigned)H * (unsigned)W, groups = HW / V;
  const long long total = (long long)N * groups;
  for (long long i = blockIdx.x * (long long)SY_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * SY_THREADS) {
    const int n = total <= 0xffffffffLL ? (int)((unsigned)i / groups) : (int)(i / groups);    // (a 64-bit division is long)
    const unsigned q = (unsigned)(i - (long long)n * groups) * V;       // first pixel of the group in its plane
    const float* px = img + (long long)n * 3 * HW + q;
    float v[3][V], mk[V];
    if (V == 4) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(px + (long long)c * HW);
        v[c][0] = t[0]; v[c][1] = t[1]; v[c][2] = t[2]; v[c][3] = t[3];
      }
      if (mask_in) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(mask_in + (long long)n * HW + q);
        mk[0] = t[0]; mk[1] = t[1]; mk[2] = t[2]; mk[3] = t[3];
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c][0] = px[(long long)c * HW];
      if (mask_in) mk[0] = mask_in[(long long)n * HW + q];
    }
    if (!mask_in) {
#pragma unroll
      for (int k = 0; k < V; ++k) mk[k] = 0.f;
    }

    const unet_synth_desc d = desc[n];
    // (the entry point has refused a batch with a descriptor outside these ranges; an image is left alone rather than
    // read out of bounds should the device copy ever differ from the host copy it was checked on)
    const bool on = d.apply != 0 && pow2_upto64(d.cells_y) && pow2_upto64(d.cells_x) && (unsigned)d.src < (unsigned)N &&
                    (unsigned)d.shift_y < (unsigned)H && (unsigned)d.shift_x < (unsigned)W && (unsigned)d.perm < 6u;
    if (on) {
      const int ly = 31 - __clz(d.cells_y), lx = 31 - __clz(d.cells_x);
      const int* yc = ycell + (long long)ly * H;
      const int* xc = xcell + (long long)lx * W;
      const float* yt = ytf + (long long)ly * 2 * H;                     // [0, H): t, [H, 2H): fade(t)
      const float* xt = xtf + (long long)lx * 2 * W;
      const unsigned code = (unsigned)(0x061209211824ULL >> (8 * d.perm));    // perm(c) = (code >> 2c) & 3
      const float* donor = img + (long long)d.src * 3 * HW;
      int y = (int)(q / (unsigned)W), x = (int)(q - (unsigned)y * (unsigned)W);
      int ciy = -1, cix = -1;
      float g00x = 0.f, g00y = 0.f, g10x = 0.f, g10y = 0.f, g01x = 0.f, g01y = 0.f, g11x = 0.f, g11y = 0.f;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const int iy = yc[y], ix = xc[x];
        if (iy != ciy || ix != cix) {
          ciy = iy; cix = ix;
          const uint32_t h00 = lattice_hash(d.seed, iy, ix) & 255u, h10 = lattice_hash(d.seed, iy, ix + 1) & 255u;
          const uint32_t h01 = lattice_hash(d.seed, iy + 1, ix) & 255u, h11 = lattice_hash(d.seed, iy + 1, ix + 1) & 255u;
          g00x = gtab[h00][0]; g00y = gtab[h00][1];
          g10x = gtab[h10][0]; g10y = gtab[h10][1];
          g01x = gtab[h01][0]; g01y = gtab[h01][1];
          g11x = gtab[h11][0]; g11y = gtab[h11][1];
        }
        const float ty = yt[y], fy = yt[H + y], tx = xt[x], fx = xt[W + x];
        const float tx1 = tx - 1.f, ty1 = ty - 1.f;
        const float d00 = g00x * tx + g00y * ty, d10 = g10x * tx1 + g10y * ty;
        const float d01 = g01x * tx + g01y * ty1, d11 = g11x * tx1 + g11y * ty1;
        const float noise = lerp1(lerp1(d00, d10, fx), lerp1(d01, d11, fx), fy) * 1.41421356237309504880f;
        if (noise > d.threshold) {
          int yy = y + d.shift_y, xx = x + d.shift_x;
          if (yy >= H) yy -= H;
          if (xx >= W) xx -= W;
          const float* dp = donor + (long long)yy * W + xx;
#pragma unroll
          for (int c = 0; c < 3; ++c)
            v[c][k] = d.beta * v[c][k] + d.one_minus_beta * dp[(long long)((code >> (2 * c)) & 3u) * HW];
          mk[k] = fmaxf(mk[k], 1.f);
        }
        if (++x == W) { x = 0; ++y; }
      }
    }

    float* po = out + (long long)n * 3 * HW + q;
    if (V == 4) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const f32x4 t = {v[c][0], v[c][1], v[c][2], v[c][3]};
        *reinterpret_cast<f32x4*>(po + (long long)c * HW) = t;
      }
      const f32x4 t = {mk[0], mk[1], mk[2], mk[3]};
      *reinterpret_cast<f32x4*>(mask_out + (long long)n * HW + q) = t;
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) po[(long long)c * HW] = v[c][0];
      mask_out[(long long)n * HW + q] = mk[0];
    }
  }
}

}  // namespace

extern "C" int32_t unet_synth_anomalies(const float* images, const float* masks_in, int32_t n, int32_t c, int32_t h,
                                        int32_t w, const unet_synth_desc* desc, const unet_synth_desc* desc_host,
                                        const int32_t* ycell, const float* ytf, const int32_t* xcell, const float* xtf,
                                        const float* gradients, float* corrupted, float* masks_out, void* stream) {
  UNET_REQUIRE(images && desc && desc_host && ycell && ytf && xcell && xtf && gradients && corrupted && masks_out,
               UNET_ERR_BAD_ARG, "unet_synth_anomalies: null pointer");
  UNET_REQUIRE(images != corrupted, UNET_ERR_BAD_ARG, "unet_synth_anomalies: in place (the donor reads the clean batch)");
  UNET_REQUIRE(c == 3, UNET_ERR_UNSUPPORTED, "unet_synth_anomalies: %d channels (RGB batches only)", c);
  UNET_REQUIRE(n > 0 && h > 0 && w > 0, UNET_ERR_UNSUPPORTED, "unet_synth_anomalies: batch %d x %d x %d", n, h, w);
  UNET_REQUIRE(h < 32768 && w < 32768, UNET_ERR_UNSUPPORTED, "unet_synth_anomalies: sides must stay below 32768");
  for (int i = 0; i < n; ++i) {
    const unet_synth_desc& d = desc_host[i];
    UNET_REQUIRE(d.src >= 0 && d.src < n, UNET_ERR_UNSUPPORTED, "unet_synth_anomalies: image %d: donor %d outside the batch",
                 i, d.src);
    const bool cells = d.cells_y >= 1 && d.cells_y <= 64 && (d.cells_y & (d.cells_y - 1)) == 0 && d.cells_x >= 1 &&
                       d.cells_x <= 64 && (d.cells_x & (d.cells_x - 1)) == 0;
    UNET_REQUIRE(cells && d.shift_y >= 0 && d.shift_y < h && d.shift_x >= 0 && d.shift_x < w && d.perm >= 0 && d.perm < 6,
                 UNET_ERR_UNSUPPORTED, "unet_synth_anomalies: image %d: cells %d x %d, shift (%d, %d), permutation %d", i,
                 d.cells_y, d.cells_x, d.shift_y, d.shift_x, d.perm);
  }
  const long long hw = (long long)h * w;
  auto aligned = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  const bool vec = hw % 4 == 0 && aligned(images) && aligned(corrupted) && aligned(masks_out) && aligned(masks_in);
  const long long threads = (long long)n * (vec ? hw / 4 : hw);
  const int blocks = (int)(cdiv64(threads, SY_THREADS) < SY_MAX_BLOCKS ? cdiv64(threads, SY_THREADS) : SY_MAX_BLOCKS);
  hipStream_t s = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(synth_kernel<4>, dim3(blocks), dim3(SY_THREADS), 0, s, images, masks_in, corrupted, masks_out, n, h, w,
                       desc, ycell, ytf, xcell, xtf, gradients);
  else
    hipLaunchKernelGGL(synth_kernel<1>, dim3(blocks), dim3(SY_THREADS), 0, s, images, masks_in, corrupted, masks_out, n, h, w,
                       desc, ycell, ytf, xcell, xtf, gradients);
  return unet_check_launch(vec ? "synth_kernel<4>" : "synth_kernel<1>");
}
