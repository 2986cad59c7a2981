// The visualisation sheet of the evaluation CLI (reference src/test.py:315-332 -> src/utils.py:111-157 visualize_results:
// original | true mask (cmap gray) | predicted map (cmap hot) | reconstruction, one row per sample, drawn there by
// matplotlib on the host).  Here the panels are rendered from the device tensors into one packed uint8 RGB sheet of N
// rows of K panels of H x W pixels, `gutter` pixels of 255 between panels in both directions, in two launches:
//   render_range   lo / hi = the smallest / largest finite value of every map plane (matplotlib's Normalize autoscale):
//                  per-block minimum and maximum of order-preserving uint32 keys (score_key, as the AUC sort), then one
//                  integer atomicMin and atomicMax per block.  No float atomics: the result does not depend on scheduling.
//   render_sheet   a thread produces RUN = 4 consecutive pixels of one sheet row = 12 bytes = 3 dwords, stored as dwords
//                  where the run is whole and its address dword-aligned, else byte by byte.  With W and the gutter both
//                  multiples of 4 a run never crosses a panel border and its inputs come in as 16-byte loads (VEC).
//                  The run geometry, the table staging and the byte / blend rules are sheet.h's, shared with segvis.hip.
// Per-pixel arithmetic (every product and sum rounds once: this file is built with -ffp-contract=off):
//   image    v = x * std[c], then + mean[c] (fp32), clamp to [0, 1], byte = (uint8)(v * 255.0f) truncating; NaN -> 0
//   unit     clamp to [0, 1], the same byte rule (the reconstruction panel)
//   gray/hot in fp64: t = ((double)x - lo) / (hi - lo), i = floor(t * 256) clipped to [0, 255], bytes = LUT[i]; hi == lo
//            gives i = 0; a non-finite pixel, and every pixel of a plane without a finite one, is (255, 255, 255).
//            fp64 subtraction, division and multiplication are correctly rounded here and in numpy, so i is the index
//            matplotlib's cmap(Normalize()(x.astype(float64))) takes, exactly; from fp32 it would differ at bin borders.
//   overlay  (a8 * hot(map) + (255 - a8) * image + 127) / 255 in integers per channel; a non-finite map pixel shows image
// The two 256-entry LUTs come from the caller (device memory, [2][256][3] bytes: gray, hot) and are staged in LDS.
#include "segpixel.h"
#include "sheet.h"

namespace {

using segpx::aligned;
using namespace sheet;                                 // RUN, WHITE, the pixel rules, stage_table, run_at (sheet.h)
constexpr int RG_THREADS = 256;
constexpr int RG_WAVES = RG_THREADS / WAVE;
constexpr int RG_MAX_BLOCKS = 2048;
constexpr int SH_THREADS = 256;                        // = LUT entries: thread t stages entry t of both tables
constexpr int SH_MAX_BLOCKS = 2048;
constexpr int MAX_PANELS = 8;

// ---- range -------------------------------------------------------------------------------------------------------------
struct RangeParams {
  const float* map[MAX_PANELS];                        // NULL: the panel has no map
  long long per;                                       // pixels of a plane
  int n;
  uint32_t* lo; uint32_t* hi;                          // [k][n] each; lo starts at 0xffffffff, hi at 0
};

// grid (blocks per plane, n, k).  Keys of finite floats lie in [0x00800000, 0xff7fffff]: the start values are no key.
template <int V>
__global__ __launch_bounds__(RG_THREADS) void render_range(const RangeParams A) {
  __shared__ uint32_t wlo[RG_WAVES], whi[RG_WAVES];
  const int c = blockIdx.z, n = blockIdx.y;
  const float* p = A.map[c];
  if (!p) return;                                      // block-uniform
  p += (long long)n * A.per;
  const long long units = A.per / V;                   // V divides per
  const long long per_b = cdiv64(units, gridDim.x);
  const long long u0 = blockIdx.x * per_b, u1 = min(u0 + per_b, units);
  uint32_t lo = 0xffffffffu, hi = 0u;
  for (long long u = u0 + threadIdx.x; u < u1; u += RG_THREADS) {
    float x[V];
    if constexpr (V == 4) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(p + 4 * u);
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = a[j];
    } else {
      x[0] = p[u];
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (finite_score(x[j])) {
        const uint32_t k = score_key(x[j]);
        lo = min(lo, k);
        hi = max(hi, k);
      }
    }
  }
#pragma unroll
  for (int m = WAVE / 2; m >= 1; m >>= 1) {
    lo = min(lo, (uint32_t)__shfl_xor(lo, m));
    hi = max(hi, (uint32_t)__shfl_xor(hi, m));
  }
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  if (lane == 0) { wlo[wave] = lo; whi[wave] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < RG_WAVES; ++w) { lo = min(lo, wlo[w]); hi = max(hi, whi[w]); }
    if (lo <= hi) {                                    // the block saw a finite pixel
      atomicMin(&A.lo[(long long)c * A.n + n], lo);
      atomicMax(&A.hi[(long long)c * A.n + n], hi);
    }
  }
}

// ---- sheet -------------------------------------------------------------------------------------------------------------
struct SheetParams {
  const float* rgb[MAX_PANELS];                        // [n][3][h][w]: image, unit, overlay
  const float* map[MAX_PANELS];                        // [n][1][h][w]: gray, hot, overlay
  int kind[MAX_PANELS], a8[MAX_PANELS];
  int K, N, H, W, g;
  float mean[3], std[3];
  const uint32_t* lo; const uint32_t* hi;              // [K][N] keys of render_range
  const uint8_t* luts;                                 // [2][256][3]
  uint8_t* out;
  uint32_t rw, runs;                                   // runs per sheet row, runs of the sheet
};

__device__ __forceinline__ uint32_t rgb_pixel(const SheetParams& A, bool denorm, float r, float g, float b) {
  if (denorm) denormalise(A.mean, A.std, r, g, b);
  return unit_byte(r) | (unit_byte(g) << 8) | (unit_byte(b) << 16);
}

// lo / hi of a plane as doubles; any = the plane has a finite pixel
struct Range { double lo, span; bool any; };
__device__ __forceinline__ Range plane_range(const SheetParams& A, int c, int r) {
  const uint32_t kl = A.lo[(long long)c * A.N + r], kh = A.hi[(long long)c * A.N + r];
  Range R;
  R.any = kl <= kh;
  R.lo = (double)score_of_key(kl);
  R.span = (double)score_of_key(kh) - R.lo;
  return R;
}
// index into a 256-entry colour table, or -1: draw the pixel as missing
__device__ __forceinline__ int map_index(float x, const Range& R) {
  if (!R.any || !finite_score(x)) return -1;
  if (!(R.span > 0.0)) return 0;
  const double s = floor((((double)x - R.lo) / R.span) * 256.0);
  return s >= 255.0 ? 255 : (s <= 0.0 ? 0 : (int)s);
}
// one pixel of panel c from its loaded values: v[0..2] the rgb input, m the map input
__device__ __forceinline__ uint32_t shade(const SheetParams& A, const uint32_t (*lut)[256], int kind, uint32_t a8,
                                          const Range& R, float v0, float v1, float v2, float m) {
  switch (kind) {
    case UNET_PANEL_IMAGE: return rgb_pixel(A, true, v0, v1, v2);
    case UNET_PANEL_UNIT: return rgb_pixel(A, false, v0, v1, v2);
    case UNET_PANEL_GRAY: { const int i = map_index(m, R); return i < 0 ? WHITE : lut[0][i]; }
    case UNET_PANEL_HOT: { const int i = map_index(m, R); return i < 0 ? WHITE : lut[1][i]; }
    default: {
      const uint32_t img = rgb_pixel(A, true, v0, v1, v2);
      const int i = map_index(m, R);
      return i < 0 ? img : blend(lut[1][i], img, a8);
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(SH_THREADS) void render_sheet(const SheetParams A) {
  __shared__ uint32_t lut[2][256];
#pragma unroll
  for (int m = 0; m < 2; ++m) stage_table(lut[m], A.luts, m * 256);     // gray, hot
  __syncthreads();
  const int SW = A.K * A.W + (A.K - 1) * A.g, ph = A.H + A.g, pw = A.W + A.g;
  const long long plane = (long long)A.H * A.W;
  for (uint32_t t = blockIdx.x * SH_THREADS + threadIdx.x; t < A.runs; t += gridDim.x * SH_THREADS) {
    const Run u = run_at(t, A.rw, SW);
    const int col0 = u.col0, r = u.row / ph, y = u.row % ph;     // r < N: row < N ph - g
    uint32_t px[RUN];
#pragma unroll
    for (int j = 0; j < RUN; ++j) px[j] = WHITE;
    if (y < A.H) {
      if constexpr (VEC) {                             // W, g multiples of 4: the run lies in one panel or one gutter
        const int c = col0 / pw, x = col0 % pw;        // c < K: col0 < K pw - g
        if (x < A.W) {
          const int kind = A.kind[c];
          const long long at = (long long)y * A.W + x;
          f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0, v2 = v0, m = v0;
          Range R{0.0, 0.0, false};
          if (A.rgb[c]) {
            const float* p = A.rgb[c] + (long long)r * 3 * plane + at;
            v0 = *reinterpret_cast<const f32x4*>(p);
            v1 = *reinterpret_cast<const f32x4*>(p + plane);
            v2 = *reinterpret_cast<const f32x4*>(p + 2 * plane);
          }
          if (A.map[c]) {
            m = *reinterpret_cast<const f32x4*>(A.map[c] + (long long)r * plane + at);
            R = plane_range(A, c, r);
          }
#pragma unroll
          for (int j = 0; j < RUN; ++j) px[j] = shade(A, lut, kind, (uint32_t)A.a8[c], R, v0[j], v1[j], v2[j], m[j]);
        }
      } else {
#pragma unroll
        for (int j = 0; j < RUN; ++j) {
          const int col = col0 + j;
          if (col >= SW) continue;
          const int c = col / pw, x = col % pw;
          if (x >= A.W) continue;
          const long long at = (long long)y * A.W + x;
          float v0 = 0.f, v1 = 0.f, v2 = 0.f, m = 0.f;
          Range R{0.0, 0.0, false};
          if (A.rgb[c]) {
            const float* p = A.rgb[c] + (long long)r * 3 * plane + at;
            v0 = p[0]; v1 = p[plane]; v2 = p[2 * plane];
          }
          if (A.map[c]) {
            m = A.map[c][(long long)r * plane + at];
            R = plane_range(A, c, r);
          }
          px[j] = shade(A, lut, A.kind[c], (uint32_t)A.a8[c], R, v0, v1, v2, m);
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

// shared checks of the two entry points: 0, or the status (error text set)
int32_t check_panels(const char* who, const unet_panel* panels, int32_t k, int32_t n, int32_t h, int32_t w) {
  UNET_REQUIRE(panels, UNET_ERR_BAD_ARG, "%s: null pointer", who);
  UNET_REQUIRE(k >= 1 && n >= 1 && h >= 1 && w >= 1, UNET_ERR_BAD_ARG, "%s: k=%d n=%d h=%d w=%d", who, k, n, h, w);
  UNET_REQUIRE(k <= MAX_PANELS, UNET_ERR_UNSUPPORTED, "%s: %d panels per row (at most %d)", who, k, MAX_PANELS);
  UNET_REQUIRE(n < 65536, UNET_ERR_UNSUPPORTED, "%s: n=%d (at most 65535 rows)", who, n);
  for (int c = 0; c < k; ++c) {
    const unet_panel& p = panels[c];
    const bool rgb = p.kind == UNET_PANEL_IMAGE || p.kind == UNET_PANEL_UNIT || p.kind == UNET_PANEL_OVERLAY;
    const bool map = p.kind == UNET_PANEL_GRAY || p.kind == UNET_PANEL_HOT || p.kind == UNET_PANEL_OVERLAY;
    UNET_REQUIRE(rgb || map, UNET_ERR_BAD_ARG, "%s: panel %d has kind %d", who, c, p.kind);
    UNET_REQUIRE((!rgb || p.rgb) && (!map || p.map), UNET_ERR_BAD_ARG, "%s: panel %d lacks an input", who, c);
    UNET_REQUIRE(p.alpha8 >= 0 && p.alpha8 <= 255, UNET_ERR_BAD_ARG, "%s: panel %d alpha8=%d", who, c, p.alpha8);
  }
  return 0;
}
inline bool has_map(const unet_panel& p) { return p.kind >= UNET_PANEL_GRAY; }
inline bool has_rgb(const unet_panel& p) { return p.kind != UNET_PANEL_GRAY && p.kind != UNET_PANEL_HOT; }

}  // namespace

extern "C" int32_t unet_render_range(const unet_panel* panels, int32_t k, int32_t n, int32_t h, int32_t w,
                                     uint32_t* keys, void* stream) {
  const int32_t bad = check_panels("unet_render_range", panels, k, n, h, w);
  if (bad) return bad;
  UNET_REQUIRE(keys, UNET_ERR_BAD_ARG, "unet_render_range: null pointer");
  hipStream_t s = (hipStream_t)stream;
  RangeParams A{};
  A.per = (long long)h * w;
  A.n = n;
  A.lo = keys;
  A.hi = keys + (size_t)k * n;
  int maps = 0;
  bool vec = A.per % 4 == 0;
  for (int c = 0; c < k; ++c) {
    if (!has_map(panels[c])) continue;
    A.map[c] = panels[c].map;
    vec = vec && aligned(A.map[c], 16);
    ++maps;
  }
  const size_t half = (size_t)k * n * sizeof(uint32_t);
  UNET_REQUIRE(hipMemsetAsync(A.lo, 0xff, half, s) == hipSuccess && hipMemsetAsync(A.hi, 0, half, s) == hipSuccess,
               UNET_ERR_LAUNCH, "unet_render_range: memset failed");
  if (!maps) return UNET_OK;
  const long long units = vec ? A.per / 4 : A.per;
  long long bpp = cdiv64(units, 4 * RG_THREADS);        // >= 4 units per lane
  const long long cap = RG_MAX_BLOCKS / ((long long)n * maps) > 0 ? RG_MAX_BLOCKS / ((long long)n * maps) : 1;
  if (bpp > cap) bpp = cap;
  const dim3 grid((unsigned)bpp, (unsigned)n, (unsigned)k);
  ProfScope prof(UNET_K_OTHER, 0.0, s, "render_range", (double)maps * n * A.per * 4.0);
  if (vec) hipLaunchKernelGGL(render_range<4>, grid, dim3(RG_THREADS), 0, s, A);
  else hipLaunchKernelGGL(render_range<1>, grid, dim3(RG_THREADS), 0, s, A);
  return unet_check_launch("render_range");
}

extern "C" int32_t unet_render_sheet(const unet_panel* panels, int32_t k, int32_t n, int32_t h, int32_t w,
                                     int32_t gutter, const float* mean3, const float* std3, const uint32_t* keys,
                                     const uint8_t* luts, uint8_t* sheet, void* stream) {
  const int32_t bad = check_panels("unet_render_sheet", panels, k, n, h, w);
  if (bad) return bad;
  UNET_REQUIRE(gutter >= 0, UNET_ERR_BAD_ARG, "unet_render_sheet: gutter=%d", gutter);
  const long long rows = (long long)n * h + (long long)(n - 1) * gutter;
  const long long cols = (long long)k * w + (long long)(k - 1) * gutter;
  UNET_REQUIRE(cols < (1LL << 31) / 3 && rows * cols * 3 < (1LL << 31), UNET_ERR_UNSUPPORTED,
               "unet_render_sheet: a sheet of %lld x %lld pixels (fewer than 2^31 bytes are supported)", rows, cols);
  UNET_REQUIRE(mean3 && std3 && keys && luts && sheet, UNET_ERR_BAD_ARG, "unet_render_sheet: null pointer");
  hipStream_t s = (hipStream_t)stream;
  SheetParams A{};
  bool vec = w % 4 == 0 && gutter % 4 == 0;
  double in_bytes = 0.0;
  for (int c = 0; c < k; ++c) {
    A.kind[c] = panels[c].kind;
    A.a8[c] = panels[c].alpha8;
    if (has_rgb(panels[c])) { A.rgb[c] = panels[c].rgb; vec = vec && aligned(A.rgb[c], 16); in_bytes += 12.0; }
    if (has_map(panels[c])) { A.map[c] = panels[c].map; vec = vec && aligned(A.map[c], 16); in_bytes += 4.0; }
  }
  A.K = k; A.N = n; A.H = h; A.W = w; A.g = gutter;
  for (int c = 0; c < 3; ++c) { A.mean[c] = mean3[c]; A.std[c] = std3[c]; }
  A.lo = keys;
  A.hi = keys + (size_t)k * n;
  A.luts = luts;
  A.out = sheet;
  A.rw = (uint32_t)cdiv64(cols, RUN);
  A.runs = (uint32_t)(rows * A.rw);
  long long blocks = cdiv64(A.runs, SH_THREADS);
  if (blocks > SH_MAX_BLOCKS) blocks = SH_MAX_BLOCKS;
  ProfScope prof(UNET_K_OTHER, 0.0, s, "render_sheet", in_bytes * n * h * w + 3.0 * rows * cols);
  if (vec) hipLaunchKernelGGL(render_sheet<true>, dim3((unsigned)blocks), dim3(SH_THREADS), 0, s, A);
  else hipLaunchKernelGGL(render_sheet<false>, dim3((unsigned)blocks), dim3(SH_THREADS), 0, s, A);
  return unet_check_launch("render_sheet");
}
