// Copy-paste crops (train_gear_paste; no reference counterpart): the image crop and the mask crop of crops.hip written
// together in ONE launch, with labelled defects of other images of the batch pasted in on the way out (Ghiasi et al.,
// CVPR 2021).  Restated in numpy int64 by tests/_paste_ref.py; the full rule stands in include/unet_hip.h.
//   image i      [h][w][3] bytes at src + src_offset[i]; its mask [h][w] bytes at masks + mask_offset[i]; (h, w) = src_hw[i]
//   crop k       desc[k] = {image, a[6]} as for unet_affine_crop_u8; dst_image[k][y][x][3], dst_mask[k][y][x]
//   pastes       crop k owns paste[paste_start[k] .. paste_start[k + 1] - 1], applied in that order, at most PS_MAX
//   base         pix = the bilinear crop of the image with `fill`, lab = the nearest crop of its mask with `ignore`
//   per paste    inside its dst box and where the base pixel is inside: (u, v) = b (x, y); a donor pixel is a MEMBER when it
//                lies in box (cut to the donor image) and its label is neither 0 nor `ignore`.  lab = the donor label when
//                the nearest pixel is a member; alpha = the bilinear weights (of 65536) of the member taps; if alpha > 0:
//                pix = (alpha d + (65536 - alpha) pix + 32768) >> 16 with d the bilinear value of the donor image.
// Guards: as crops.hip's, per buffer: a base image that is not readable is all `fill`, a base mask that is not readable all
// `ignore`, and a crop with either takes no paste; a paste whose donor index, image or mask is not readable is skipped;
// paste indices are clamped into [0, n_pastes), a descending paste_start owns nothing.  Members are loaded inside the
// box, which is cut to the image, and taps are clamped: no load leaves src[0, src_bytes) or masks[0, mask_bytes).
// A gather, shaped as crops.hip's: a block works on a segment of ONE output row of one crop, so descriptors, guards and
// the test of the row and segment against a paste's dst box are wave-uniform: a block no paste touches does the base
// work only.  No division by a run-time value, no atomics, no LDS, no floating point.  V = pixels per lane: 4 (three
// dword stores for the image, one for the mask) when out_w % 4 == 0 and both outputs are 4-byte aligned, else 1 (bytes).
// Measured (profiles/README.md): 32 crops of 512 x 512 take 127 us without pastes, 1.19 times the two crops.hip launches
// this one replaces, and 161 us with 2 pastes on every crop.
#include "common.h"
#include "croptaps.h"

namespace {

constexpr int PS_THREADS = 256;
constexpr int PS_MAX_BLOCKS = 16384;                   // beyond it the blocks stride over the crops
constexpr int PS_MAX_SIDE = 4096;                      // out_h, out_w
constexpr int PS_MAX_COUNT = 65535;                    // n_crops, n_images
constexpr int PS_MAX = 8;                              // UNET_PASTE_MAX: pastes looked at per crop

struct PasteParams {
  const uint8_t* src; long long src_bytes;
  const long long* src_offset; const int32_t* src_hw;
  const uint8_t* masks; long long mask_bytes; const long long* mask_offset;
  const unet_crop_desc* desc;
  const int32_t* paste_start; const unet_paste_desc* paste;
  uint8_t* dst_image; uint8_t* dst_mask;
  int n_images, n_crops, n_pastes, out_h, out_w, fill, ignore;
};

// crops.hip's readability test: does [h][w][c] at `off` lie inside a buffer of `bytes`?
__device__ __forceinline__ bool readable(long long off, int h, int w, int c, long long bytes) {
  return off >= 0 && h > 0 && w > 0 && off <= bytes && (long long)h * w <= (bytes - off) / c;
}

// a donor cut to its box: which pixels are members
struct Donor {
  const uint8_t* mask;
  int w, x0, y0, x1, y1, ignore;
  __device__ __forceinline__ unsigned label(long long px, long long py) const {      // 0: not a member
    if (px < x0 || px >= x1 || py < y0 || py >= y1) return 0u;
    const unsigned m = mask[py * w + px];
    return m == (unsigned)ignore ? 0u : m;
  }
};

template <int V>
__global__ __launch_bounds__(PS_THREADS) void paste_crop(const PasteParams P) {
  const int seg_x0 = (int)blockIdx.x * (int)blockDim.x * V, seg_x1 = seg_x0 + (int)blockDim.x * V;     // uniform
  const int xl = seg_x0 + (int)threadIdx.x * V;
  if (xl >= P.out_w) return;
  const int y = (int)blockIdx.y;
  for (int k = (int)blockIdx.z; k < P.n_crops; k += (int)gridDim.z) {
    const unet_crop_desc d = P.desc[k];                // uniform
    // the guards, uniform: a buffer the tables do not place an image in is never read
    bool img_ok = false, msk_ok = false;
    long long off = 0, moff = 0;
    int h = 0, w = 0;
    if (d.image >= 0 && d.image < P.n_images) {
      off = P.src_offset[d.image];
      moff = P.mask_offset[d.image];
      h = P.src_hw[2 * d.image];
      w = P.src_hw[2 * d.image + 1];
      img_ok = readable(off, h, w, 3, P.src_bytes);
      msk_ok = readable(moff, h, w, 1, P.mask_bytes);
    }
    const uint8_t* img = P.src + (img_ok ? off : 0);
    const uint8_t* msk = P.masks + (msk_ok ? moff : 0);
    const long long uy = (long long)d.a[1] * y + d.a[2], vy = (long long)d.a[4] * y + d.a[5];

    unsigned pix[V][3], lab[V];
    bool in[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int x = xl + j;
      const long long u = (long long)d.a[0] * x + uy, v = (long long)d.a[3] * x + vy;
      Taps t = taps_of<1>(u, v, h, w, 3);
      Taps tm = taps_of<0>(u, v, h, w, 1);
      in[j] = t.inside && img_ok && msk_ok;
      t.inside = t.inside && img_ok;
      tm.inside = tm.inside && msk_ok;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) pix[j][ch] = sample<1>(img, t, ch, P.fill);
      lab[j] = sample<0>(msk, tm, 0, P.ignore);
    }

    if (P.n_pastes > 0 && img_ok && msk_ok) {          // uniform
      const long long first = P.paste_start[k];
      long long count = (long long)P.paste_start[k + 1] - first;
      count = count > PS_MAX ? PS_MAX : count;
      for (long long i = 0; i < count; ++i) {
        long long j = first + i;
        j = j < 0 ? 0 : (j >= P.n_pastes ? P.n_pastes - 1 : j);
        const unet_paste_desc p = P.paste[j];          // uniform
        if (y < p.dst[1] || y >= p.dst[3] || seg_x1 <= p.dst[0] || seg_x0 >= p.dst[2]) continue;       // not this block
        if (p.image < 0 || p.image >= P.n_images) continue;
        const long long doff = P.src_offset[p.image], dmoff = P.mask_offset[p.image];
        const int dh = P.src_hw[2 * p.image], dw = P.src_hw[2 * p.image + 1];
        if (!readable(doff, dh, dw, 3, P.src_bytes) || !readable(dmoff, dh, dw, 1, P.mask_bytes)) continue;
        const uint8_t* dimg = P.src + doff;
        Donor D;
        D.mask = P.masks + dmoff;
        D.w = dw;
        D.ignore = P.ignore;
        D.x0 = p.box[0] < 0 ? 0 : p.box[0];
        D.y0 = p.box[1] < 0 ? 0 : p.box[1];
        D.x1 = p.box[2] > dw ? dw : p.box[2];
        D.y1 = p.box[3] > dh ? dh : p.box[3];
        if (D.x0 >= D.x1 || D.y0 >= D.y1) continue;
        const long long puy = (long long)p.b[1] * y + p.b[2], pvy = (long long)p.b[4] * y + p.b[5];
#pragma unroll
        for (int q = 0; q < V; ++q) {
          const int x = xl + q;
          if (!in[q] || x < p.dst[0] || x >= p.dst[2]) continue;
          const long long u = (long long)p.b[0] * x + puy, v = (long long)p.b[3] * x + pvy;
          const unsigned m = D.label(u >> 16, v >> 16);
          if (m) lab[q] = m;
          // a tap is a member by its own position, before the clamp: a tap outside the donor image is none
          const long long tx = (u - 32768) >> 16, ty = (v - 32768) >> 16;
          Taps t;
          t.inside = true;
          bilinear_taps(t, u, v, dh, dw, 3);
          const int gx = 256 - t.fx, gy = 256 - t.fy;
          int alpha = 0;
          if (D.label(tx, ty)) alpha += gx * gy;
          if (D.label(tx + 1, ty)) alpha += t.fx * gy;
          if (D.label(tx, ty + 1)) alpha += gx * t.fy;
          if (D.label(tx + 1, ty + 1)) alpha += t.fx * t.fy;
          if (alpha > 0) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
              const unsigned dv = sample<1>(dimg, t, ch, 0);
              pix[q][ch] = ((unsigned)alpha * dv + (unsigned)(65536 - alpha) * pix[q][ch] + 32768u) >> 16;
            }
          }
        }
      }
    }

    const long long row = (long long)k * P.out_h + y;
    uint8_t* oi = P.dst_image + (row * P.out_w + xl) * 3;
    uint8_t* om = P.dst_mask + row * P.out_w + xl;
    if constexpr (V == 4) {
      uint32_t* wi = reinterpret_cast<uint32_t*>(oi);
      wi[0] = pix[0][0] | pix[0][1] << 8 | pix[0][2] << 16 | pix[1][0] << 24;
      wi[1] = pix[1][1] | pix[1][2] << 8 | pix[2][0] << 16 | pix[2][1] << 24;
      wi[2] = pix[2][2] | pix[3][0] << 8 | pix[3][1] << 16 | pix[3][2] << 24;
      *reinterpret_cast<uint32_t*>(om) = lab[0] | lab[1] << 8 | lab[2] << 16 | lab[3] << 24;
    } else {
      oi[0] = (uint8_t)pix[0][0]; oi[1] = (uint8_t)pix[0][1]; oi[2] = (uint8_t)pix[0][2];
      *om = (uint8_t)lab[0];
    }
  }
}

}  // namespace

extern "C" int32_t unet_paste_crop_u8(const uint8_t* src, int64_t src_bytes, const int64_t* src_offset,
                                      const int32_t* src_hw, int32_t n_images, const uint8_t* masks, int64_t mask_bytes,
                                      const int64_t* mask_offset, const unet_crop_desc* desc, int32_t n_crops,
                                      const int32_t* paste_start, const unet_paste_desc* paste, int32_t n_pastes,
                                      int32_t out_h, int32_t out_w, int32_t fill, int32_t ignore, uint8_t* dst_image,
                                      uint8_t* dst_mask, void* stream) {
  const char* who = "unet_paste_crop_u8";
  static_assert(sizeof(unet_paste_desc) == 64 && PS_MAX == UNET_PASTE_MAX, "unet_paste_desc");
  UNET_REQUIRE(src && src_offset && src_hw && masks && mask_offset && desc && paste_start && dst_image && dst_mask,
               UNET_ERR_BAD_ARG, "%s: null pointer", who);
  UNET_REQUIRE(n_pastes >= 0, UNET_ERR_UNSUPPORTED, "%s: n_pastes %d (at least 0)", who, n_pastes);
  UNET_REQUIRE(paste || n_pastes == 0, UNET_ERR_BAD_ARG, "%s: null pointer (paste, with n_pastes %d)", who, n_pastes);
  UNET_REQUIRE(fill >= 0 && fill <= 255, UNET_ERR_UNSUPPORTED, "%s: fill %d (0..255)", who, fill);
  UNET_REQUIRE(ignore >= 0 && ignore <= 255, UNET_ERR_UNSUPPORTED, "%s: ignore %d (0..255)", who, ignore);
  UNET_REQUIRE(out_h >= 1 && out_h <= PS_MAX_SIDE && out_w >= 1 && out_w <= PS_MAX_SIDE, UNET_ERR_UNSUPPORTED,
               "%s: crops of %d x %d (sides 1..%d)", who, out_h, out_w, PS_MAX_SIDE);
  UNET_REQUIRE(n_crops >= 1 && n_crops <= PS_MAX_COUNT, UNET_ERR_UNSUPPORTED, "%s: %d crops (1..%d)", who, n_crops,
               PS_MAX_COUNT);
  UNET_REQUIRE(n_images >= 1 && n_images <= PS_MAX_COUNT, UNET_ERR_UNSUPPORTED, "%s: %d images (1..%d)", who, n_images,
               PS_MAX_COUNT);
  UNET_REQUIRE(src_bytes > 0, UNET_ERR_UNSUPPORTED, "%s: src_bytes %lld (at least 1)", who, (long long)src_bytes);
  UNET_REQUIRE(mask_bytes > 0, UNET_ERR_UNSUPPORTED, "%s: mask_bytes %lld (at least 1)", who, (long long)mask_bytes);
  const bool words = out_w % 4 == 0 && ((uintptr_t)dst_image & 3) == 0 && ((uintptr_t)dst_mask & 3) == 0;
  const int units = words ? out_w / 4 : out_w;         // lanes a row needs
  const int segs = cdiv(units, PS_THREADS);            // <= 16; the row's lanes spread evenly over them, in whole waves
  const unsigned threads = (unsigned)(cdiv(cdiv(units, segs), WAVE) * WAVE);
  int gz = PS_MAX_BLOCKS / (segs * out_h);
  gz = gz < 1 ? 1 : (gz > n_crops ? n_crops : gz);
  const PasteParams P{src, (long long)src_bytes, (const long long*)src_offset, src_hw, masks, (long long)mask_bytes,
                      (const long long*)mask_offset, desc, paste_start, paste, dst_image, dst_mask, n_images, n_crops,
                      n_pastes, out_h, out_w, fill, ignore};
  const dim3 grid((unsigned)segs, (unsigned)out_h, (unsigned)gz), block(threads);
  hipStream_t s = (hipStream_t)stream;
  const double out_bytes = (double)n_crops * out_h * out_w * 4.0;
  ProfScope prof(UNET_K_OTHER, 0.0, s, "paste_crop", 2.0 * out_bytes);
  if (words) hipLaunchKernelGGL((paste_crop<4>), grid, block, 0, s, P);
  else hipLaunchKernelGGL((paste_crop<1>), grid, block, 0, s, P);
  return unet_check_launch("paste_crop");
}
