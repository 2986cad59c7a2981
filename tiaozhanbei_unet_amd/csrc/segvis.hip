// Prediction pictures of the Gear / KolektorSDD visualisation CLIs (reference visualize.py, visualize_kolektorsdd.py,
// drawn there by matplotlib on the host from tensors copied off the device), rendered from the device tensors:
//   seg_confidence     labels = argmax over classes (first maximum, strict >: torch.argmax / seg_stats_kernel) and
//                      conf = softmax(logits).max(0) = 1 / sum_j expf(z_j - z_max) per pixel, all in fp32, j in class
//                      order (visualize.py:134-135, visualize_kolektorsdd.py:131).  A lane owns 4 consecutive pixels (one
//                      16-byte read per class plane, one 4-byte label store, one 16-byte confidence store) when hw % 4 == 0
//                      and the pointers allow it, else 1 pixel.  HBM-bound, no reductions, no atomics.  The rule itself
//                      is segpixel.h's argmax_conf, which tiles.hip and views.hip apply to their merged logits.
//   seg_confidence_scaled  the same kernel with SCALED (eval_calibration): conf = 1 / sum_j expf((z_j - z_max) * inv_t), the
//                      labels still those of the raw logits; inv_t == 1 gives seg_confidence's bytes.
//   seg_render_sheet   one launch writes the whole uint8 RGB sheet of ceil(n / per_row) rows of per_row samples of k panels
//                      of h x w pixels, `gutter` pixels of 255 between panels in both directions and in the cells past n.
//                      The run geometry, the table staging and the pixel rules are sheet.h's, shared with render.hip.  With
//                      w and the gutter both multiples of 4 a run never crosses a panel border and its inputs come in as
//                      16-byte (image, map) and 4-byte (labels) loads (VEC).
// Per-pixel arithmetic (every product and sum rounds once: this file is built with -ffp-contract=off):
//   image    sheet.h's denormalise and unit_byte, render.hip's UNET_PANEL_IMAGE: v = x * std[c], then + mean[c] (fp32), clamp to
//            [0, 1], NaN -> 0, byte = (uint8)(v * 255.0f) truncating
//   classes  palette[label]
//   overlay  label 0: the image byte (visualize.py:112-113 draws nothing on the background); else
//            (a8 * palette[label] + (255 - a8) * image + 127) / 255 in integers per channel (sheet.h's blend)
//   lut      the fixed range [0, 1] of imshow(vmin=0, vmax=1): i = floor(v * 256) (exact in fp32) clipped to [0, 255],
//            v < 0 gives 0; a non-finite pixel is (255, 255, 255)
// The two 256-entry tables (class palette, colour map) come from the caller in device memory and are staged in LDS.
#include "segpixel.h"
#include "sheet.h"

namespace {

using namespace segpx;                                 // MAXC, aligned, argmax_conf (segpixel.h)
using namespace sheet;                                 // RUN, WHITE, the pixel rules, stage_table, run_at (sheet.h)
constexpr int CF_THREADS = 256;
constexpr int CF_MAX_BLOCKS = 4096;
constexpr int SH_THREADS = 256;                        // = table entries: thread t stages entry t of both tables
constexpr int SH_MAX_BLOCKS = 2048;
constexpr int MAX_PANELS = 8;

// ---- confidence --------------------------------------------------------------------------------------------------------
struct ConfParams {
  const float* logits; unsigned char* labels; float* conf;
  int C; float inv_t; long long hw;                    // inv_t: read by the SCALED kernels only
  long long units;                                     // n * hw / V
};

// grid-stride over units of V pixels; V divides hw, so a unit lies in one image.  SCALED: the confidence at the
// temperature 1 / inv_t (unet_seg_confidence_scaled)
template <int V, bool SCALED>
__global__ __launch_bounds__(CF_THREADS) void seg_confidence(const ConfParams P) {
  const long long per_img = P.hw / V;
  for (long long u = (long long)blockIdx.x * CF_THREADS + threadIdx.x; u < P.units; u += (long long)gridDim.x * CF_THREADS) {
    const long long n = u / per_img, at = (u % per_img) * V;
    const float* x = P.logits + n * P.C * P.hw + at;
    float z[V][MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      if (c < P.C) {
        if constexpr (V == 4) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(x + c * P.hw);
          z[0][c] = v[0]; z[1][c] = v[1]; z[2][c] = v[2]; z[3][c] = v[3];
        } else {
          z[0][c] = x[c * P.hw];
        }
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) z[j][c] = 0.f;
      }
    }
    int arg[V];
    float cf[V];
#pragma unroll
    for (int j = 0; j < V; ++j) arg[j] = argmax_conf<SCALED>(z[j], P.C, cf[j], P.inv_t);
    const long long o = n * P.hw + at;
    if constexpr (V == 4) {
      if (P.labels)
        *reinterpret_cast<unsigned int*>(P.labels + o) =
            (unsigned)arg[0] | ((unsigned)arg[1] << 8) | ((unsigned)arg[2] << 16) | ((unsigned)arg[3] << 24);
      if (P.conf) {
        const f32x4 v = {cf[0], cf[1], cf[2], cf[3]};
        *reinterpret_cast<f32x4*>(P.conf + o) = v;
      }
    } else {
      if (P.labels) P.labels[o] = (unsigned char)arg[0];
      if (P.conf) P.conf[o] = cf[0];
    }
  }
}

// both entry points after their checks: 4 pixels per lane when hw % 4 == 0 and the pointers allow it, else 1
template <bool SCALED>
int32_t launch_confidence(const char* name, const float* logits, int n, int c, long long hw, float inv_t, uint8_t* labels,
                          float* conf, hipStream_t s) {
  const bool vec = hw % 4 == 0 && aligned(logits, 16) && (!labels || aligned(labels, 4)) && (!conf || aligned(conf, 16));
  ConfParams P{logits, labels, conf, c, inv_t, hw, (long long)n * (hw / (vec ? 4 : 1))};
  long long blocks = cdiv64(P.units, CF_THREADS);
  if (blocks > CF_MAX_BLOCKS) blocks = CF_MAX_BLOCKS;
  const double bytes = (double)n * hw * (4.0 * c + (labels ? 1.0 : 0.0) + (conf ? 4.0 : 0.0));
  ProfScope prof(UNET_K_OTHER, 0.0, s, name, bytes);
  if (vec) hipLaunchKernelGGL((seg_confidence<4, SCALED>), dim3((unsigned)blocks), dim3(CF_THREADS), 0, s, P);
  else hipLaunchKernelGGL((seg_confidence<1, SCALED>), dim3((unsigned)blocks), dim3(CF_THREADS), 0, s, P);
  return unet_check_launch(name);
}

// ---- sheet -------------------------------------------------------------------------------------------------------------
struct SheetParams {
  const float* image;                                  // [n][3][h][w]
  const unsigned char* labels[MAX_PANELS];             // [n][h][w]: classes, overlay
  const float* map[MAX_PANELS];                        // [n][h][w]: lut
  int kind[MAX_PANELS], a8[MAX_PANELS];
  int K, N, H, W, g, per_row;
  float mean[3], std[3];
  const uint8_t* palette; const uint8_t* lut;          // [256][3] each
  uint8_t* out;
  int SW;                                              // sheet width in pixels
  uint32_t rw, runs;                                   // runs per sheet row, runs of the sheet
};

__device__ __forceinline__ uint32_t image_pixel(const SheetParams& A, float r, float g, float b) {
  denormalise(A.mean, A.std, r, g, b);
  return unit_byte(r) | (unit_byte(g) << 8) | (unit_byte(b) << 16);
}
// one pixel of a panel from its loaded values: v0..v2 the image input, l the label, m the map input
__device__ __forceinline__ uint32_t shade(const SheetParams& A, const uint32_t* pal, const uint32_t* lut, int kind,
                                          uint32_t a8, float v0, float v1, float v2, uint32_t l, float m) {
  switch (kind) {
    case UNET_SEG_PANEL_IMAGE: return image_pixel(A, v0, v1, v2);
    case UNET_SEG_PANEL_CLASSES: return pal[l];
    case UNET_SEG_PANEL_OVERLAY: {
      const uint32_t img = image_pixel(A, v0, v1, v2);
      return l == 0 ? img : blend(pal[l], img, a8);
    }
    default: {
      if (!finite_score(m)) return WHITE;
      const float s = floorf(m * 256.0f);
      return lut[s >= 255.0f ? 255 : (s <= 0.0f ? 0 : (int)s)];
    }
  }
}
__device__ __forceinline__ bool needs_image(int kind) { return kind == UNET_SEG_PANEL_IMAGE || kind == UNET_SEG_PANEL_OVERLAY; }

template <bool VEC>
__global__ __launch_bounds__(SH_THREADS) void seg_render_sheet(const SheetParams A) {
  __shared__ uint32_t tab[2][256];                     // palette, colour map
  stage_table(tab[0], A.palette);
  stage_table(tab[1], A.lut);
  __syncthreads();
  const int SW = A.SW, ph = A.H + A.g, pw = A.W + A.g;
  const long long plane = (long long)A.H * A.W;
  for (uint32_t t = blockIdx.x * SH_THREADS + threadIdx.x; t < A.runs; t += gridDim.x * SH_THREADS) {
    const Run u = run_at(t, A.rw, SW);
    const int col0 = u.col0, r = u.row / ph, y = u.row % ph;     // r < R: row < R ph - g
    uint32_t px[RUN];
#pragma unroll
    for (int j = 0; j < RUN; ++j) px[j] = WHITE;
    if (y < A.H) {
      if constexpr (VEC) {                             // W, g multiples of 4: the run lies in one panel or one gutter
        const int cell = col0 / pw, x = col0 % pw;     // cell < per_row K: col0 < per_row K pw - g
        const int i = r * A.per_row + cell / A.K, c = cell % A.K;
        if (x < A.W && i < A.N) {
          const int kind = A.kind[c];
          const long long at = (long long)i * plane + (long long)y * A.W + x;
          f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0, v2 = v0, m = v0;
          uint32_t l4 = 0;
          if (needs_image(kind)) {
            const float* p = A.image + 2 * (long long)i * plane + at;     // (3 i planes + the pixel)
            v0 = *reinterpret_cast<const f32x4*>(p);
            v1 = *reinterpret_cast<const f32x4*>(p + plane);
            v2 = *reinterpret_cast<const f32x4*>(p + 2 * plane);
          }
          if (A.labels[c]) l4 = *reinterpret_cast<const uint32_t*>(A.labels[c] + at);
          if (A.map[c]) m = *reinterpret_cast<const f32x4*>(A.map[c] + at);
#pragma unroll
          for (int j = 0; j < RUN; ++j)
            px[j] = shade(A, tab[0], tab[1], kind, (uint32_t)A.a8[c], v0[j], v1[j], v2[j], (l4 >> (8 * j)) & 255u, m[j]);
        }
      } else {
#pragma unroll
        for (int j = 0; j < RUN; ++j) {
          const int col = col0 + j;
          if (col >= SW) continue;
          const int cell = col / pw, x = col % pw;
          const int i = r * A.per_row + cell / A.K, c = cell % A.K;
          if (x >= A.W || i >= A.N) continue;
          const int kind = A.kind[c];
          const long long at = (long long)i * plane + (long long)y * A.W + x;
          float v0 = 0.f, v1 = 0.f, v2 = 0.f, m = 0.f;
          uint32_t l = 0;
          if (needs_image(kind)) {
            const float* p = A.image + 2 * (long long)i * plane + at;
            v0 = p[0]; v1 = p[plane]; v2 = p[2 * plane];
          }
          if (A.labels[c]) l = A.labels[c][at];
          if (A.map[c]) m = A.map[c][at];
          px[j] = shade(A, tab[0], tab[1], kind, (uint32_t)A.a8[c], v0, v1, v2, l, m);
        }
      }
    }
    // 4 pixels x 3 bytes, the first pixel's red in the lowest byte
    const uint32_t w[3] = {px[0] | (px[1] << 24), (px[1] >> 8) | (px[2] << 16), (px[2] >> 16) | (px[3] << 8)};
    uint8_t* a = A.out + (long long)u.row * (3LL * SW) + 3LL * col0;
    if (u.cnt == RUN && ((uintptr_t)a & 3u) == 0) {
      uint32_t* q = reinterpret_cast<uint32_t*>(a);
      q[0] = w[0]; q[1] = w[1]; q[2] = w[2];
    } else {
#pragma unroll
      for (int j = 0; j < 3 * RUN; ++j)
        if (j < 3 * u.cnt) a[j] = (uint8_t)(w[j / 4] >> (8 * (j % 4)));
    }
  }
}

}  // namespace

extern "C" int32_t unet_seg_confidence(const float* logits, int32_t n, int32_t c, int64_t hw, uint8_t* labels,
                                       float* conf, void* stream) {
  UNET_REQUIRE(logits && (labels || conf), UNET_ERR_BAD_ARG, "unet_seg_confidence: null pointer");
  UNET_REQUIRE(n > 0 && hw > 0 && c >= 2 && c <= MAXC, UNET_ERR_UNSUPPORTED,
               "unet_seg_confidence: n=%d c=%d hw=%lld (2..8 classes)", n, c, (long long)hw);
  return launch_confidence<false>("seg_confidence", logits, n, c, hw, 1.0f, labels, conf, (hipStream_t)stream);
}

// seg_confidence at a temperature (eval_calibration): conf = 1 / sum_j expf((z_j - z_max) * inv_t), the labels those of
// the raw logits; inv_t == 1 gives unet_seg_confidence's bytes
extern "C" int32_t unet_seg_confidence_scaled(const float* logits, int32_t n, int32_t c, int64_t hw, float inv_t,
                                              uint8_t* labels, float* conf, void* stream) {
  const char* who = "unet_seg_confidence_scaled";
  UNET_REQUIRE(logits && (labels || conf), UNET_ERR_UNSUPPORTED, "%s: null pointer", who);
  UNET_REQUIRE(n > 0 && hw > 0 && c >= 2 && c <= MAXC, UNET_ERR_UNSUPPORTED, "%s: n=%d c=%d hw=%lld (2..8 classes)", who, n,
               c, (long long)hw);
  UNET_REQUIRE(inv_t > 0.0f && inv_t <= 3.402823466e38f, UNET_ERR_UNSUPPORTED, "%s: inv_t=%g is not a finite value > 0", who,
               (double)inv_t);
  return launch_confidence<true>("seg_confidence_scaled", logits, n, c, hw, inv_t, labels, conf, (hipStream_t)stream);
}

extern "C" int32_t unet_seg_render_sheet(const float* image, const unet_seg_panel* panels, int32_t k, int32_t n,
                                         int32_t h, int32_t w, int32_t gutter, int32_t per_row, const float* mean3,
                                         const float* std3, const uint8_t* palette, const uint8_t* lut, uint8_t* sheet,
                                         void* stream) {
  const char* who = "unet_seg_render_sheet";
  UNET_REQUIRE(panels, UNET_ERR_BAD_ARG, "%s: null pointer", who);
  UNET_REQUIRE(k >= 1 && n >= 1 && h >= 1 && w >= 1 && gutter >= 0 && per_row >= 1, UNET_ERR_BAD_ARG,
               "%s: k=%d n=%d h=%d w=%d gutter=%d per_row=%d", who, k, n, h, w, gutter, per_row);
  UNET_REQUIRE(k <= MAX_PANELS, UNET_ERR_UNSUPPORTED, "%s: %d panels per sample (at most %d)", who, k, MAX_PANELS);
  UNET_REQUIRE(n < 65536, UNET_ERR_UNSUPPORTED, "%s: n=%d (at most 65535 samples)", who, n);
  const long long R = cdiv64(n, per_row), cells = (long long)per_row * k;
  const long long rows = R * h + (R - 1) * gutter, cols = cells * w + (cells - 1) * gutter;
  UNET_REQUIRE(cols < (1LL << 31) / 3 && rows * cols * 3 < (1LL << 31), UNET_ERR_UNSUPPORTED,
               "%s: a sheet of %lld x %lld pixels (fewer than 2^31 bytes are supported)", who, rows, cols);
  UNET_REQUIRE(mean3 && std3 && palette && lut && sheet, UNET_ERR_BAD_ARG, "%s: null pointer", who);
  hipStream_t s = (hipStream_t)stream;
  SheetParams A{};
  bool vec = w % 4 == 0 && gutter % 4 == 0, any_image = false;
  double in_bytes = 0.0;
  for (int c = 0; c < k; ++c) {
    const unet_seg_panel& p = panels[c];
    UNET_REQUIRE(p.kind >= UNET_SEG_PANEL_IMAGE && p.kind <= UNET_SEG_PANEL_LUT, UNET_ERR_BAD_ARG,
                 "%s: panel %d has kind %d", who, c, p.kind);
    const bool lab = p.kind == UNET_SEG_PANEL_CLASSES || p.kind == UNET_SEG_PANEL_OVERLAY;
    const bool map = p.kind == UNET_SEG_PANEL_LUT;
    UNET_REQUIRE((!lab || p.labels) && (!map || p.map), UNET_ERR_BAD_ARG, "%s: panel %d lacks an input", who, c);
    UNET_REQUIRE(p.alpha8 >= 0 && p.alpha8 <= 255, UNET_ERR_BAD_ARG, "%s: panel %d alpha8=%d", who, c, p.alpha8);
    A.kind[c] = p.kind;
    A.a8[c] = p.alpha8;
    if (p.kind == UNET_SEG_PANEL_IMAGE || p.kind == UNET_SEG_PANEL_OVERLAY) { any_image = true; in_bytes += 12.0; }
    if (lab) { A.labels[c] = p.labels; vec = vec && aligned(p.labels, 4); in_bytes += 1.0; }
    if (map) { A.map[c] = p.map; vec = vec && aligned(p.map, 16); in_bytes += 4.0; }
  }
  UNET_REQUIRE(!any_image || image, UNET_ERR_BAD_ARG, "%s: an image or overlay panel without the image", who);
  if (any_image) vec = vec && aligned(image, 16);
  A.image = image;
  A.K = k; A.N = n; A.H = h; A.W = w; A.g = gutter; A.per_row = per_row;
  for (int c = 0; c < 3; ++c) { A.mean[c] = mean3[c]; A.std[c] = std3[c]; }
  A.palette = palette;
  A.lut = lut;
  A.out = sheet;
  A.SW = (int)cols;
  A.rw = (uint32_t)cdiv64(cols, RUN);
  A.runs = (uint32_t)(rows * A.rw);
  long long blocks = cdiv64(A.runs, SH_THREADS);
  if (blocks > SH_MAX_BLOCKS) blocks = SH_MAX_BLOCKS;
  ProfScope prof(UNET_K_OTHER, 0.0, s, "seg_render_sheet", in_bytes * n * h * w + 3.0 * rows * cols);
  if (vec) hipLaunchKernelGGL(seg_render_sheet<true>, dim3((unsigned)blocks), dim3(SH_THREADS), 0, s, A);
  else hipLaunchKernelGGL(seg_render_sheet<false>, dim3((unsigned)blocks), dim3(SH_THREADS), 0, s, A);
  return unet_check_launch("seg_render_sheet");
}
