// 8-connected regions of the ground-truth masks (truth > 0.5) with their sizes: what the per-region-overlap (PRO) curve
// of the MVTec evaluation weights its pixels by.  Tiled union-find on parent links (index of a pixel of the same region
// with a smaller or equal linear index y*w + x; a root links to itself), four launches, no workgroup waits on another:
//   label_tile     a 32x32 tile in LDS: every defective pixel is united with its W neighbour and with N, or (N clear)
//                  NW and NE, by atomicMin on the links; each pixel then finds its tile root.  Writes the root's image
//                  index as the pixel's global link and, at the root, the pixel count of the tile component.
//   merge_borders  a thread per pixel of a tile's first column / first row: united with its (up to 3) neighbours in
//                  the tile to the left / above by atomicMin on the global links.
//   root_sizes     every tile root finds its region root, adds its count there (integer atomicAdd) and links to it.
//   finish         every pixel: label = 1 + region root, size = the root's count; the totals {regions, defective, ok}.
// A link only ever decreases and always stays inside its region, so a stale read costs a retry, never a wrong union;
// the minimum index of a region is its only possible root, so labels and sizes are a function of the mask alone.
#include "unionfind.h"

namespace {

using namespace uf;                                   // tiles, links, find_root, unite (unionfind.h)
constexpr int FIN_ITEMS = 8;                           // pixels per lane of finish_labels: 3 count atomics per 2048 pixels

struct LabelParams {
  const float* truth; const uint8_t* select;
  int h, w, tiles_x, tiles_y;
  long long per;                                       // h * w
  int* parent; int* labels; int* sizes;
  unsigned long long* counts;                          // {regions, defective, ok}
};

__global__ __launch_bounds__(LT_THREADS) void label_tile(const LabelParams A) {
  __shared__ int par[LT_PIX];
  __shared__ int cnt[LT_PIX];
  const int n = blockIdx.y;
  if (A.select && !A.select[n]) return;                // block-uniform
  const int y0 = (int)(blockIdx.x / A.tiles_x) * LT, x0 = (int)(blockIdx.x % A.tiles_x) * LT;
  const float* t = A.truth + (long long)n * A.per;
  constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
  bool def[LT_ITEMS];
#pragma unroll
  for (int j = 0; j < LT_ITEMS; ++j) {
    const int i = threadIdx.x + j * LT_THREADS, y = y0 + i / LT, x = x0 + i % LT;
    def[j] = y < A.h && x < A.w && t[(long long)y * A.w + x] > 0.5f;
    par[i] = def[j] ? i : -1;
    cnt[i] = 0;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < LT_ITEMS; ++j) {
    if (!def[j]) continue;
    const int i = threadIdx.x + j * LT_THREADS, ly = i / LT, lx = i % LT;
    if (lx > 0 && link_of<WG>(par, i - 1) >= 0) unite<WG>(par, i, i - 1);
    if (ly > 0) {
      if (link_of<WG>(par, i - LT) >= 0) {             // N joins NW and NE by their own W links
        unite<WG>(par, i, i - LT);
      } else {
        if (lx > 0 && link_of<WG>(par, i - LT - 1) >= 0) unite<WG>(par, i, i - LT - 1);
        if (lx < LT - 1 && link_of<WG>(par, i - LT + 1) >= 0) unite<WG>(par, i, i - LT + 1);
      }
    }
  }
  __syncthreads();
  int root[LT_ITEMS];
#pragma unroll
  for (int j = 0; j < LT_ITEMS; ++j) {
    root[j] = def[j] ? find_root<WG>(par, threadIdx.x + j * LT_THREADS) : -1;
    if (def[j]) atomicAdd(&cnt[root[j]], 1);
  }
  __syncthreads();
  int* parent = A.parent + (long long)n * A.per;
  int* sizes = A.sizes + (long long)n * A.per;
#pragma unroll
  for (int j = 0; j < LT_ITEMS; ++j) {
    const int i = threadIdx.x + j * LT_THREADS, y = y0 + i / LT, x = x0 + i % LT;
    if (y >= A.h || x >= A.w) continue;
    const long long g = (long long)y * A.w + x;
    // the tile's row-major order follows the image's: the tile root is the component's smallest image index too
    parent[g] = def[j] ? (y0 + root[j] / LT) * A.w + x0 + root[j] % LT : -1;
    sizes[g] = root[j] == i ? cnt[i] : 0;
  }
}

// grid (border pixels of one image / PX_THREADS, images): first the (tiles_x - 1) * h pixels of the tiles' first
// columns, then the (tiles_y - 1) * w pixels of their first rows
__global__ __launch_bounds__(PX_THREADS) void merge_borders(const LabelParams A) {
  const int n = blockIdx.y;
  if (A.select && !A.select[n]) return;
  constexpr int DEV = __HIP_MEMORY_SCOPE_AGENT;
  const long long cols = (long long)(A.tiles_x - 1) * A.h, rows = (long long)(A.tiles_y - 1) * A.w;
  long long b = (long long)blockIdx.x * PX_THREADS + threadIdx.x;
  if (b >= cols + rows) return;
  int* parent = A.parent + (long long)n * A.per;
  int x, y, dx, dy;                                    // the neighbours are (x - 1 + k dx, y - 1 + k dy), k = 0, 1, 2
  if (b < cols) {
    x = (int)(b / A.h + 1) * LT; y = (int)(b % A.h); dx = 0; dy = 1;
  } else {
    b -= cols;
    y = (int)(b / A.w + 1) * LT; x = (int)(b % A.w); dx = 1; dy = 0;
  }
  const int p = y * A.w + x;
  if (link_of<DEV>(parent, p) < 0) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int qx = x - 1 + k * dx, qy = y - 1 + k * dy;
    if (qx < 0 || qy < 0 || qx >= A.w || qy >= A.h) continue;
    const int q = qy * A.w + qx;
    if (link_of<DEV>(parent, q) >= 0) unite<DEV>(parent, p, q);
  }
}

// grid (pixels of one image / PX_THREADS, images).  Only region roots are added to and only they are read by other
// threads (sign only: a tile root's count is positive from the start), so the adds need no second array.
__global__ __launch_bounds__(PX_THREADS) void root_sizes(const LabelParams A) {
  const int n = blockIdx.y;
  if (A.select && !A.select[n]) return;
  const long long g = (long long)blockIdx.x * PX_THREADS + threadIdx.x;
  if (g >= A.per) return;
  int* parent = A.parent + (long long)n * A.per;
  int* sizes = A.sizes + (long long)n * A.per;
  add_tile_root(parent, sizes, (int)g);
}

__global__ __launch_bounds__(PX_THREADS) void finish_labels(const LabelParams A) {
  __shared__ unsigned int red[3][PX_THREADS / WAVE];
  const int n = blockIdx.y;
  const bool on = !A.select || A.select[n];            // block-uniform
  unsigned int c[3] = {0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < FIN_ITEMS; ++k) {
    const long long g = ((long long)blockIdx.x * FIN_ITEMS + k) * PX_THREADS + threadIdx.x;
    if (g >= A.per) break;
    const long long o = (long long)n * A.per + g;
    int label = 0, size = 0;
    if (on) {
      const int* parent = A.parent + (long long)n * A.per;
      if (parent[g] >= 0) {
        const int r = find_root<__HIP_MEMORY_SCOPE_AGENT>(parent, (int)g);   // at most tile root -> region root
        label = r + 1;
        size = A.sizes[(long long)n * A.per + r];      // a root's entry is never written here
        c[0] += r == (int)g; c[1] += 1u;
      } else {
        c[2] += 1u;
      }
    }
    A.labels[o] = label;
    if (label != (int)g + 1) A.sizes[o] = size;
  }
  if (!on) return;
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) c[k] += __shfl_xor(c[k], m);
    if (lane == 0) red[k][wave] = c[k];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long tot = 0;
#pragma unroll
    for (int w = 0; w < PX_THREADS / WAVE; ++w) tot += red[threadIdx.x][w];
    if (tot) atomicAdd(&A.counts[threadIdx.x], tot);
  }
}

inline bool supported(int64_t n, int64_t h, int64_t w) { return frames_supported(n, h, w); }

}  // namespace

extern "C" size_t unet_label_regions_workspace(int64_t n, int64_t h, int64_t w) {
  if (!supported(n, h, w)) return 0;
  return up16((size_t)(n * h * w) * 4);
}

extern "C" int32_t unet_label_regions(const float* truth, const uint8_t* select, int64_t n, int64_t h, int64_t w,
                                      int32_t* labels, int32_t* sizes, int64_t* counts, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  UNET_REQUIRE(truth && labels && sizes && counts && workspace, UNET_ERR_BAD_ARG, "unet_label_regions: null pointer");
  UNET_REQUIRE(n > 0 && h > 0 && w > 0, UNET_ERR_BAD_ARG, "unet_label_regions: n=%lld h=%lld w=%lld", (long long)n,
               (long long)h, (long long)w);
  UNET_REQUIRE(supported(n, h, w), UNET_ERR_UNSUPPORTED,
               "unet_label_regions: n=%lld h=%lld w=%lld (n < 65536 and at most 2^31 - 1 pixels)", (long long)n,
               (long long)h, (long long)w);
  UNET_REQUIRE(workspace_bytes >= unet_label_regions_workspace(n, h, w), UNET_ERR_WORKSPACE,
               "unet_label_regions: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int tx = (int)cdiv64(w, LT), ty = (int)cdiv64(h, LT);
  LabelParams A{truth, select, (int)h, (int)w, tx, ty, (long long)(h * w), (int*)workspace, labels, sizes,
                (unsigned long long*)counts};
  ProfScope prof(UNET_K_OTHER, 0.0, s, "label_tile", (double)n * h * w * 12.0);
  hipLaunchKernelGGL(label_tile, dim3((unsigned)((long long)tx * ty), (unsigned)n), dim3(LT_THREADS), 0, s, A);
  int32_t rc = unet_check_launch("label_tile");
  if (rc) return rc;
  const long long border = (long long)(tx - 1) * h + (long long)(ty - 1) * w;
  if (border > 0) {
    hipLaunchKernelGGL(merge_borders, dim3((unsigned)cdiv64(border, PX_THREADS), (unsigned)n), dim3(PX_THREADS), 0, s, A);
    rc = unet_check_launch("merge_borders");
    if (rc) return rc;
  }
  const dim3 grid((unsigned)cdiv64(h * w, PX_THREADS), (unsigned)n);
  if (border > 0) {                                    // one tile: every tile root is a region root already
    hipLaunchKernelGGL(root_sizes, grid, dim3(PX_THREADS), 0, s, A);
    rc = unet_check_launch("root_sizes");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(finish_labels, dim3((unsigned)cdiv64(h * w, PX_THREADS * FIN_ITEMS), (unsigned)n), dim3(PX_THREADS),
                     0, s, A);
  return unet_check_launch("finish_labels");
}
