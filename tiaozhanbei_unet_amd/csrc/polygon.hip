// Gear label masks on the GPU: LabelMe polygons -> uint8 class masks, rasterised directly at the sample points of the
// NEAREST resize.  Restates, per output pixel, what /root/reference/src/gear_dataset.py:112-201 + :241-259 compute on
// the host: every polygon drawn with ImageDraw.polygon(xy, fill=1) into its own full-resolution image, OR-ed per raw
// class, priority resolved (spalling raw 1 -> 2 over pitting raw 0 -> 1 over scrape raw 2 -> 3), then
// Image.resize((out_w, out_h), NEAREST).
//
// Pillow's polygon fill (Draw.c polygon_generic, 8-bit images), as inferred from Pillow 12.2.0's output and pinned by
// tests/golden/gear_masks.npz (the corner rule below is a reconstruction, not Pillow's code; see "Known divergence"):
//   - edges in vertex order, closing edge only when the last vertex differs from the first;
//   - a horizontal edge (y0 == y1) is drawn as the line [xmin, xmax] on its row;
//   - every other edge with ymin <= y <= ymax crosses scan line y at x = float((y - y0) * dx + x0), dx = float(x1 - x0) /
//     (y1 - y0), every product and sum rounded once (no fused multiply-add: this file is built with -ffp-contract=off);
//   - at its lower end (y == ymax) an edge counts twice unless y is the polygon's last row;
//   - a "corner" fix-up: an integral crossing at an end point of its edge that meets an earlier edge with the same
//     slope sign at one of that edge's end points (same x) is moved next to where the two edges are on the adjacent row;
//   - crossings sorted, paired, each pair (a, b) fills [ROUND_UP(a), ROUND_DOWN(b)] (Draw.c's float macros).
// The host keeps parsing (the reference's int(float(tok) * size) truncation) and the random draws.
//
// Known divergence: Pillow applies its corner fix-up under a condition not fully reconstructed here.  Polygons that
// revisit a vertex (A, B, A, C ...) can differ from Pillow by a few pixels on the revisited vertex's row; the fixture's
// "diverge_*" cases pin that gap.  Every other fixture case, LabelMe-like blobs at 1920 x 1080 included, is bit-exact.
//
// Layout: one 256-thread workgroup per (output row, image).  Each wave takes every fourth polygon of the image, computes
// that polygon's crossings of the row's source scan line one edge per lane, compacts them into its LDS buffer with
// ballots, rank-sorts them, and marks the covered output columns of the row in its own LDS class-bit row.  No wave
// writes another wave's LDS and nothing is atomic: the output does not depend on scheduling.
//
// polygon_class_histogram_kernel (the class-overlap census of a label set) runs the same per-row, per-polygon body at
// the native resolution and, in place of the priority step, counts the row's eight possible class-bit sets.
#include <limits.h>
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr int kMaxCross = 1024;           // crossings of one polygon on one row: <= 2 per edge -> <= 512 vertices
constexpr int kMaxVertices = kMaxCross / 2;
constexpr int kMaxOutW = 4096;

struct Edge {
  int x0, y0, x1, y1;
};

__device__ __forceinline__ Edge load_edge(const int* __restrict__ v, int first, int nv, int e) {
  const int a = first + e, b = first + (e + 1 < nv ? e + 1 : 0);
  return Edge{v[2 * a], v[2 * a + 1], v[2 * b], v[2 * b + 1]};
}

__device__ __forceinline__ float edge_dx(const Edge& e) {
  return __fdiv_rn((float)(e.x1 - e.x0), (float)(e.y1 - e.y0));
}

// (y - y0) * dx + x0 as Draw.c evaluates it: int difference converted to float, float product, float sum
__device__ __forceinline__ float edge_x(const Edge& e, float dx, int y) {
  return __fadd_rn(__fmul_rn((float)(y - e.y0), dx), (float)e.x0);
}

// Draw.c ROUND_UP / ROUND_DOWN: the +-0.5F is a float operation, floor / ceil then act on that float
__device__ __forceinline__ int round_up(float f) {
  return f >= 0.0f ? (int)floorf(__fadd_rn(f, 0.5f)) : -(int)floorf(__fadd_rn(fabsf(f), 0.5f));
}
__device__ __forceinline__ int round_down(float f) {
  return f >= 0.0f ? (int)ceilf(__fsub_rn(f, 0.5f)) : -(int)ceilf(__fsub_rn(fabsf(f), 0.5f));
}

// C roundf: halves away from zero
__device__ __forceinline__ float c_roundf(float f) { return roundf(f); }

// crossing(s) of edge e (index ei in vertex order) with scan line y; returns how many (0, 1 or 2) were written to x[]
__device__ int edge_crossings(const int* __restrict__ v, int first, int nv, int ei, int y, int poly_ymax, float x[2]) {
  const Edge e = load_edge(v, first, nv, ei);
  const int ylo = min(e.y0, e.y1), yhi = max(e.y0, e.y1);
  if (ylo == yhi || y < ylo || y > yhi) return 0;
  const float dx = edge_dx(e);
  float xc = edge_x(e, dx, y);
  if (y == yhi && y < poly_ymax) {          // "needed to draw consistent polygons": the lower end counts twice
    x[0] = x[1] = xc;
    return 2;
  }
  if (dx != 0.0f && rintf(xc) == xc && (y == ylo || y == yhi)) {
    // connect a corner with an earlier edge that ends on this row at the same x with a slope of the same sign
    for (int k = 0; k < ei; ++k) {
      const Edge o = load_edge(v, first, nv, k);
      const int olo = min(o.y0, o.y1), ohi = max(o.y0, o.y1);
      if (olo == ohi || (y != olo && y != ohi)) continue;
      const float odx = edge_dx(o);
      if ((dx > 0.0f && odx <= 0.0f) || (dx < 0.0f && odx >= 0.0f)) continue;
      if (xc != edge_x(o, odx, y)) continue;
      const int y2 = y + (y == yhi ? -1 : 1);
      if (y2 < olo || y2 > ohi) continue;
      const float a = edge_x(e, dx, y2), b = edge_x(o, odx, y2);
      if (xc > __fadd_rn(a, 1.0f) && xc > __fadd_rn(b, 1.0f)) {
        xc = __fadd_rn(c_roundf(fmaxf(a, b)), 1.0f);
      } else if (xc < __fsub_rn(a, 1.0f) && xc < __fsub_rn(b, 1.0f)) {
        xc = __fsub_rn(c_roundf(fminf(a, b)), 1.0f);
      }
      break;
    }
  }
  x[0] = xc;
  return 1;
}

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

// which source column an output column samples: the sibling kernels differ only in this
struct TableColumns {                                // NEAREST resize: the image's index table (-1 = outside)
  const int* __restrict__ xrow;
  __device__ __forceinline__ int operator()(int j) const { return xrow[j]; }
};
struct IdentityColumns {                             // native resolution
  __device__ __forceinline__ int operator()(int j) const { return j; }
};

// polygons [lower_bound, upper_bound) of image img (poly_img is non-decreasing), found by one thread
__device__ __forceinline__ void image_polygon_range(const int* __restrict__ poly_img, int n_polys, int img, int* prange) {
  int lo = 0, hi = n_polys;
  while (lo < hi) { const int m = (lo + hi) >> 1; if (poly_img[m] < img) lo = m + 1; else hi = m; }
  int lo2 = lo, hi2 = n_polys;
  while (lo2 < hi2) { const int m = (lo2 + hi2) >> 1; if (poly_img[m] <= img) lo2 = m + 1; else hi2 = m; }
  prange[0] = lo;
  prange[1] = lo2;
}

// One wave, one polygon p, one source scan line sy: ORs the polygon's class bit into bits[j] for every output column
// j < out_w whose source column cols(j) the polygon's fill covers.  xbuf / sbuf / hspan / bits are this wave's own LDS.
template <class Columns>
__device__ __forceinline__ void mark_polygon_row(const int* __restrict__ verts, const int* __restrict__ poly_off,
                                                 const int* __restrict__ poly_cls, int p, int sy, int src_w, int out_w,
                                                 const Columns cols, int lane, float* xbuf, float* sbuf, int* hspan,
                                                 unsigned char* bits) {
  const int cls = poly_cls[p];
  if (cls < 0 || cls > 2) return;                    // the reference's final loop visits raw classes 2, 0 and 1 only
  const int first = poly_off[p], nv = poly_off[p + 1] - first;
  if (nv < 3 || nv > kMaxVertices) return;           // (the host rejects both)
  int ymin = INT_MAX, ymax = INT_MIN;
  for (int i = lane; i < nv; i += 64) {
    const int yv = verts[2 * (first + i) + 1];
    ymin = min(ymin, yv);
    ymax = max(ymax, yv);
  }
  for (int s = 32; s > 0; s >>= 1) {
    ymin = min(ymin, __shfl_xor(ymin, s));
    ymax = max(ymax, __shfl_xor(ymax, s));
  }
  if (sy < ymin || sy > ymax) return;                // wave-uniform
  const bool closed = verts[2 * (first + nv - 1)] == verts[2 * first] &&
                      verts[2 * (first + nv - 1) + 1] == verts[2 * first + 1];
  const int ne = closed ? nv - 1 : nv;

  // 1. crossings, compacted in edge order (the fix-up above only looks at earlier edges' geometry, not at the buffer)
  int nx = 0;
  for (int base = 0; base < ne; base += 64) {
    const int ei = base + lane;
    float xc[2];
    const int c = ei < ne ? edge_crossings(verts, first, nv, ei, sy, ymax, xc) : 0;
    const unsigned long long b1 = __ballot(c >= 1), b2 = __ballot(c == 2);
    const int pos = nx + __popcll(b1 & lanes_below(lane)) + __popcll(b2 & lanes_below(lane));
    if (c >= 1 && pos < kMaxCross) xbuf[pos] = xc[0];
    if (c == 2 && pos + 1 < kMaxCross) xbuf[pos + 1] = xc[1];
    nx += __popcll(b1) + __popcll(b2);
  }
  nx = min(nx, kMaxCross);
  __builtin_amdgcn_wave_barrier();
  // 2. rank sort (ties by position: a stable order, and equal values are interchangeable anyway)
  for (int t = lane; t < nx; t += 64) {
    const float xt = xbuf[t];
    int r = 0;
    for (int u = 0; u < nx; ++u) {
      const float xu = xbuf[u];
      r += (xu < xt) || (xu == xt && u < t);
    }
    sbuf[r] = xt;
  }
  __builtin_amdgcn_wave_barrier();
  // 3. horizontal edges on this row, drawn as lines [xmin, xmax]: compacted as int pairs
  int nh = 0;
  for (int base = 0; base < ne; base += 64) {
    const int ei = base + lane;
    bool h = false;
    Edge e{0, 0, 0, 0};
    if (ei < ne) {
      e = load_edge(verts, first, nv, ei);
      h = e.y0 == e.y1 && e.y0 == sy;
    }
    const unsigned long long bh = __ballot(h);
    const int pos = nh + __popcll(bh & lanes_below(lane));
    if (h && 2 * pos + 1 < kMaxCross) {
      hspan[2 * pos] = min(e.x0, e.x1);
      hspan[2 * pos + 1] = max(e.x0, e.x1);
    }
    nh += __popcll(bh);
  }
  nh = min(nh, kMaxCross / 2);
  __builtin_amdgcn_wave_barrier();
  // 4. mark the output columns whose source column lies in a filled span
  const unsigned char bit = (unsigned char)(1u << cls);
  for (int j = lane; j < out_w; j += 64) {
    const int sx = cols(j);
    if (sx < 0 || sx >= src_w) continue;
    bool hit = false;
    for (int m = 1; m < nx && !hit; m += 2) hit = round_up(sbuf[m - 1]) <= sx && sx <= round_down(sbuf[m]);
    for (int m = 0; m < nh && !hit; ++m) hit = hspan[2 * m] <= sx && sx <= hspan[2 * m + 1];
    if (hit) bits[j] |= bit;
  }
  __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(kThreads) void polygon_mask_u8_kernel(
    const int* __restrict__ verts, const int* __restrict__ poly_off, const int* __restrict__ poly_cls,
    const int* __restrict__ poly_img, int n_polys, const int* __restrict__ src_hw, int out_h, int out_w,
    const int* __restrict__ yidx, const int* __restrict__ xidx, unsigned char* __restrict__ dst) {
  __shared__ float xbuf[kWaves][kMaxCross];         // unsorted crossings
  __shared__ float sbuf[kWaves][kMaxCross];         // sorted crossings
  __shared__ int hbuf[kWaves][kMaxCross];           // horizontal-edge spans [xmin, xmax]: <= 1 per edge
  __shared__ unsigned char bits[kWaves][kMaxOutW];  // per-wave class bits of the output row: 1 raw0, 2 raw1, 4 raw2
  __shared__ int prange[2];

  const int row = blockIdx.x, img = blockIdx.y;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int src_h = src_hw[2 * img], src_w = src_hw[2 * img + 1];
  const int sy = yidx[(long long)img * out_h + row];
  const TableColumns cols{xidx + (long long)img * out_w};
  unsigned char* out = dst + ((long long)img * out_h + row) * out_w;

  for (int j = tid; j < kWaves * out_w; j += kThreads) bits[j / out_w][j % out_w] = 0;
  if (tid == 0) image_polygon_range(poly_img, n_polys, img, prange);
  __syncthreads();
  const bool row_inside = sy >= 0 && sy < src_h;

  for (int p = prange[0] + wave; row_inside && p < prange[1]; p += kWaves)
    mark_polygon_row(verts, poly_off, poly_cls, p, sy, src_w, out_w, cols, lane, xbuf[wave], sbuf[wave], hbuf[wave],
                     bits[wave]);
  __syncthreads();
  // 5. priority: raw 1 (spalling) -> 2, raw 0 (pitting) -> 1, raw 2 (scrape) -> 3
  for (int j = tid; j < out_w; j += kThreads) {
    unsigned b = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) b |= bits[w][j];
    out[j] = (b & 2) ? 2 : (b & 1) ? 1 : (b & 4) ? 3 : 0;
  }
}

// Class-overlap census: hist[img][b] = number of pixels of image img, at its native size, whose set of covering raw
// classes is exactly b (bit c set = some class-c polygon covers the pixel).  One workgroup per (source row, image) over
// rows 0 .. max_h - 1; the same marking as above with identity columns, then the row's eight counts by ballots per wave,
// summed over the waves in LDS and added to the image's eight bins with 64-bit integer atomics (exact in any order).
__global__ __launch_bounds__(kThreads) void polygon_class_histogram_kernel(
    const int* __restrict__ verts, const int* __restrict__ poly_off, const int* __restrict__ poly_cls,
    const int* __restrict__ poly_img, int n_polys, const int* __restrict__ src_hw, int max_w,
    unsigned long long* __restrict__ hist) {
  __shared__ float xbuf[kWaves][kMaxCross];
  __shared__ float sbuf[kWaves][kMaxCross];
  __shared__ int hbuf[kWaves][kMaxCross];
  __shared__ unsigned char bits[kWaves][kMaxOutW];
  __shared__ int prange[2];
  __shared__ int wcount[kWaves][8];                 // per-wave counts of the row's eight bit sets

  const int sy = blockIdx.x, img = blockIdx.y;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int src_h = src_hw[2 * img], src_w = src_hw[2 * img + 1];
  // a row beyond this image's height contributes nothing; nor does an image wider than the caller declared (the bit
  // rows hold max_w <= kMaxOutW columns).  Both are uniform over the workgroup.
  if (sy >= src_h || src_w <= 0 || src_w > max_w || src_w > kMaxOutW) return;

  for (int j = tid; j < src_w; j += kThreads) {
#pragma unroll
    for (int w = 0; w < kWaves; ++w) bits[w][j] = 0;
  }
  if (tid == 0) image_polygon_range(poly_img, n_polys, img, prange);
  __syncthreads();

  for (int p = prange[0] + wave; p < prange[1]; p += kWaves)
    mark_polygon_row(verts, poly_off, poly_cls, p, sy, src_w, src_w, IdentityColumns{}, lane, xbuf[wave], sbuf[wave],
                     hbuf[wave], bits[wave]);
  __syncthreads();

  int count[8] = {0, 0, 0, 0, 0, 0, 0, 0};          // wave-uniform
  for (int base = wave * 64; base < src_w; base += kThreads) {
    const int j = base + lane;
    unsigned b = 0;
    if (j < src_w) {
#pragma unroll
      for (int w = 0; w < kWaves; ++w) b |= bits[w][j];
    }
    const unsigned long long in = __ballot(j < src_w);
    const unsigned long long m0 = __ballot((b & 1) != 0), m1 = __ballot((b & 2) != 0), m2 = __ballot((b & 4) != 0);
#pragma unroll
    for (int v = 0; v < 8; ++v)
      count[v] += __popcll(in & ((v & 1) ? m0 : ~m0) & ((v & 2) ? m1 : ~m1) & ((v & 4) ? m2 : ~m2));
  }
  if (lane == 0) {
#pragma unroll
    for (int v = 0; v < 8; ++v) wcount[wave][v] = count[v];
  }
  __syncthreads();
  if (tid < 8) {
    int total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) total += wcount[w][tid];
    if (total) atomicAdd(hist + (long long)img * 8 + tid, (unsigned long long)total);
  }
}

}  // namespace

extern "C" int32_t unet_polygon_mask_u8(const int32_t* verts, const int32_t* poly_offsets, const int32_t* poly_class,
                                        const int32_t* poly_image, int32_t n_polys, int32_t max_poly_vertices,
                                        const int32_t* src_hw, int32_t n, int32_t out_h, int32_t out_w,
                                        const int32_t* yidx, const int32_t* xidx, uint8_t* dst, void* stream) {
  UNET_REQUIRE(dst && src_hw && yidx && xidx && n > 0 && out_h > 0 && out_w > 0 && n_polys >= 0, UNET_ERR_BAD_ARG,
               "unet_polygon_mask_u8: bad argument");
  UNET_REQUIRE(n_polys == 0 || (verts && poly_offsets && poly_class && poly_image), UNET_ERR_BAD_ARG,
               "unet_polygon_mask_u8: polygon arrays missing");
  UNET_REQUIRE(out_w <= kMaxOutW && n <= 65535, UNET_ERR_UNSUPPORTED, "unet_polygon_mask_u8: out_w <= %d, n <= 65535",
               kMaxOutW);
  UNET_REQUIRE(max_poly_vertices <= kMaxVertices, UNET_ERR_UNSUPPORTED,
               "unet_polygon_mask_u8: polygons of at most %d vertices", kMaxVertices);
  hipLaunchKernelGGL(polygon_mask_u8_kernel, dim3(out_h, n), dim3(kThreads), 0, (hipStream_t)stream, verts, poly_offsets,
                     poly_class, poly_image, n_polys, src_hw, out_h, out_w, yidx, xidx, dst);
  return unet_check_launch("polygon_mask_u8_kernel");
}

extern "C" int32_t unet_polygon_class_histogram(const int32_t* verts, const int32_t* poly_offsets,
                                                const int32_t* poly_class, const int32_t* poly_image, int32_t n_polys,
                                                int32_t max_poly_vertices, const int32_t* src_hw, int32_t n,
                                                int32_t max_h, int32_t max_w, int64_t* hist, void* stream) {
  UNET_REQUIRE(hist && src_hw && n > 0 && max_h > 0 && max_w > 0 && n_polys >= 0 && max_poly_vertices >= 0,
               UNET_ERR_BAD_ARG, "unet_polygon_class_histogram: bad argument");
  UNET_REQUIRE(n_polys == 0 || (verts && poly_offsets && poly_class && poly_image), UNET_ERR_BAD_ARG,
               "unet_polygon_class_histogram: polygon arrays missing");
  UNET_REQUIRE(max_w <= kMaxOutW && n <= 65535, UNET_ERR_UNSUPPORTED,
               "unet_polygon_class_histogram: src_w <= %d for every image, n <= 65535", kMaxOutW);
  UNET_REQUIRE(max_poly_vertices <= kMaxVertices, UNET_ERR_UNSUPPORTED,
               "unet_polygon_class_histogram: polygons of at most %d vertices", kMaxVertices);
  UNET_REQUIRE(hipMemsetAsync(hist, 0, (size_t)n * 8 * sizeof(int64_t), (hipStream_t)stream) == hipSuccess,
               UNET_ERR_LAUNCH, "unet_polygon_class_histogram: memset failed");
  hipLaunchKernelGGL(polygon_class_histogram_kernel, dim3(max_h, n), dim3(kThreads), 0, (hipStream_t)stream, verts,
                     poly_offsets, poly_class, poly_image, n_polys, src_hw, max_w, (unsigned long long*)hist);
  return unet_check_launch("polygon_class_histogram_kernel");
}
