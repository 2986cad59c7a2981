// Affine crops of a ragged batch (train_gear_crops; no reference counterpart: the reference squeezes every image into the
// trainer's frame): any number of crops of ONE size, cut with scale, rotation and flip out of images of DIFFERENT sizes
// that lie packed in one byte buffer, in one launch.  Restated in numpy int64 by tests/_crops_ref.py.
//   image i      [h][w][c] bytes at src + src_offset[i], (h, w) = src_hw[i]
//   crop k       desc[k] = {image, a[6]}: the matrix in 16.16 fixed point, a2 / a5 holding the half-pixel terms
//                (unet_flip_rotate_u8's convention); dst[k][y][x][ch]
//   per pixel    u = a0 x + a1 y + a2, v = a3 x + a4 y + a5 (int64); nx = u >> 16, ny = v >> 16 (floor).  Inside iff
//                0 <= nx < w and 0 <= ny < h, in BOTH modes; outside every channel is `fill`.
//   nearest      dst = src[ny][nx][ch]
//   bilinear     ub = u - 32768, x0 = ub >> 16, fx = (ub & 0xFFFF) >> 8, x1 = x0 + 1, both clamped to [0, w - 1]; the same
//                along y; top = (256 - fx) p00 + fx p01, bot likewise; dst = ((256 - fy) top + fy bot + 32768) >> 16.
//                Integers only: the bytes are a function of the inputs alone, and a matrix that maps pixel centres to
//                pixel centres (fx = fy = 0) copies bytes.
// Guards: a crop whose image index is outside 0..n_images-1, or whose image does not lie inside src[0, src_bytes)
// (src_offset < 0, a side <= 0, src_offset + h w c > src_bytes, tested without overflow), is written as all `fill`;
// every tap of every other crop is clamped into its image.  So whatever the device tables hold, no load leaves
// src[0, src_bytes) and no store leaves dst.
// A gather.  A block works on a segment of ONE output row of one crop (grid: segment x row x crop), so the descriptor,
// the image's table entries and the guards are wave-uniform (scalar loads), a y term is formed once per row, and nothing
// is divided by a run-time value.  Two store paths: when a row's out_w c bytes are a multiple of 4 and dst is 4-byte
// aligned a lane assembles 4 consecutive bytes of the row (4 pixels of c = 1; bytes of up to 2 pixels of c = 3) and
// stores one dword, a wave 256 contiguous bytes; otherwise a lane stores one byte, a wave 64 contiguous bytes.  The taps
// are byte-wide loads, four per output byte of a bilinear crop; measured (profiles/README.md) the kernel writes 0.3 to
// 0.4 TB/s, far from the HBM rate, which costs a trainer step 0.1 ms per 32 crops of 512 x 512.
#include "common.h"
#include "croptaps.h"                              // Taps, taps_of, sample: shared with paste.hip

namespace {

constexpr int CR_THREADS = 256;
constexpr int CR_MAX_BLOCKS = 16384;                   // beyond it the blocks stride over the crops
constexpr int CR_MAX_SIDE = 4096;                      // out_h, out_w
constexpr int CR_MAX_COUNT = 65535;                    // n_crops, n_images

struct CropParams {
  const uint8_t* src; long long src_bytes;
  const long long* src_offset; const int32_t* src_hw;
  const unet_crop_desc* desc;
  uint8_t* dst;
  int n_images, n_crops, out_h, out_w, fill;
};

// blockIdx.x = segment of the row, blockIdx.y = output row y, blockIdx.z strides over the crops: no division by a
// run-time value anywhere.  C = channels; V = bytes of the row a lane writes: 4 (one dword) or 1.
template <int MODE, int V, int C>
__global__ __launch_bounds__(CR_THREADS) void affine_crop(const CropParams P) {
  const int row_bytes = P.out_w * C;
  const int b0 = ((int)blockIdx.x * (int)blockDim.x + (int)threadIdx.x) * V;
  if (b0 >= row_bytes) return;
  const int y = (int)blockIdx.y;
  for (int k = (int)blockIdx.z; k < P.n_crops; k += (int)gridDim.z) {
    const unet_crop_desc d = P.desc[k];                // uniform
    uint8_t* out = P.dst + ((long long)k * P.out_h + y) * row_bytes + b0;
    // the guards, uniform: an image the tables do not place inside src[0, src_bytes) is never read
    bool ok = d.image >= 0 && d.image < P.n_images;
    long long off = 0;
    int h = 0, w = 0;
    if (ok) {
      off = P.src_offset[d.image];
      h = P.src_hw[2 * d.image];
      w = P.src_hw[2 * d.image + 1];
      ok = off >= 0 && h > 0 && w > 0 && off <= P.src_bytes && (long long)h * w <= (P.src_bytes - off) / C;
    }
    if (!ok) {
      if constexpr (V == 4) *reinterpret_cast<uint32_t*>(out) = 0x01010101u * (unsigned)P.fill;
      else *out = (uint8_t)P.fill;
      continue;
    }
    const uint8_t* img = P.src + off;
    const long long uy = (long long)d.a[1] * y + d.a[2], vy = (long long)d.a[4] * y + d.a[5];
    if constexpr (V == 4) {
      unsigned word = 0;
      int x_held = -1;
      Taps t{};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int b = b0 + j, x = b / C, ch = b - x * C;
        if (x != x_held) {
          t = taps_of<MODE>((long long)d.a[0] * x + uy, (long long)d.a[3] * x + vy, h, w, C);
          x_held = x;
        }
        word |= sample<MODE>(img, t, ch, P.fill) << (8 * j);
      }
      *reinterpret_cast<uint32_t*>(out) = word;
    } else {
      const int x = b0 / C, ch = b0 - x * C;
      const Taps t = taps_of<MODE>((long long)d.a[0] * x + uy, (long long)d.a[3] * x + vy, h, w, C);
      *out = (uint8_t)sample<MODE>(img, t, ch, P.fill);
    }
  }
}

template <int V, int C>
void launch(int mode, dim3 grid, dim3 block, hipStream_t s, const CropParams& P) {
  if (mode) hipLaunchKernelGGL((affine_crop<1, V, C>), grid, block, 0, s, P);
  else hipLaunchKernelGGL((affine_crop<0, V, C>), grid, block, 0, s, P);
}

}  // namespace

extern "C" int32_t unet_affine_crop_u8(const uint8_t* src, int64_t src_bytes, const int64_t* src_offset,
                                       const int32_t* src_hw, int32_t n_images, int32_t c, const unet_crop_desc* desc,
                                       int32_t n_crops, int32_t out_h, int32_t out_w, int32_t mode, int32_t fill,
                                       uint8_t* dst, void* stream) {
  const char* who = "unet_affine_crop_u8";
  UNET_REQUIRE(src && src_offset && src_hw && desc && dst, UNET_ERR_BAD_ARG, "%s: null pointer", who);
  UNET_REQUIRE(c == 1 || c == 3, UNET_ERR_UNSUPPORTED, "%s: c=%d (1 or 3 channels)", who, c);
  UNET_REQUIRE(mode == 0 || mode == 1, UNET_ERR_UNSUPPORTED, "%s: mode %d (0 nearest, 1 bilinear)", who, mode);
  UNET_REQUIRE(fill >= 0 && fill <= 255, UNET_ERR_UNSUPPORTED, "%s: fill %d (0..255)", who, fill);
  UNET_REQUIRE(out_h >= 1 && out_h <= CR_MAX_SIDE && out_w >= 1 && out_w <= CR_MAX_SIDE, UNET_ERR_UNSUPPORTED,
               "%s: crops of %d x %d (sides 1..%d)", who, out_h, out_w, CR_MAX_SIDE);
  UNET_REQUIRE(n_crops >= 1 && n_crops <= CR_MAX_COUNT, UNET_ERR_UNSUPPORTED, "%s: %d crops (1..%d)", who, n_crops,
               CR_MAX_COUNT);
  UNET_REQUIRE(n_images >= 1 && n_images <= CR_MAX_COUNT, UNET_ERR_UNSUPPORTED, "%s: %d images (1..%d)", who, n_images,
               CR_MAX_COUNT);
  UNET_REQUIRE(src_bytes > 0, UNET_ERR_UNSUPPORTED, "%s: src_bytes %lld (at least 1)", who, (long long)src_bytes);
  const int row_bytes = out_w * c;                     // <= 12288
  const bool words = row_bytes % 4 == 0 && ((uintptr_t)dst & 3) == 0;
  const int units = words ? row_bytes / 4 : row_bytes;
  const int segs = cdiv(units, CR_THREADS);            // <= 48; the row's units spread evenly over them, in whole waves
  const unsigned threads = (unsigned)(cdiv(cdiv(units, segs), WAVE) * WAVE);
  int gz = CR_MAX_BLOCKS / (segs * out_h);
  gz = gz < 1 ? 1 : (gz > n_crops ? n_crops : gz);
  const CropParams P{src, (long long)src_bytes, (const long long*)src_offset, src_hw, desc, dst, n_images, n_crops, out_h,
                     out_w, fill};
  const dim3 grid((unsigned)segs, (unsigned)out_h, (unsigned)gz), block(threads);
  hipStream_t s = (hipStream_t)stream;
  const double out_bytes = (double)n_crops * out_h * row_bytes;
  ProfScope prof(UNET_K_OTHER, 0.0, s, "affine_crop", 2.0 * out_bytes);
  if (words) { if (c == 3) launch<4, 3>(mode, grid, block, s, P); else launch<4, 1>(mode, grid, block, s, P); }
  else { if (c == 3) launch<1, 3>(mode, grid, block, s, P); else launch<1, 1>(mode, grid, block, s, P); }
  return unet_check_launch("affine_crop");
}
