// 8-connected regions of the ground-truth masks (truth > 0.5) with their sizes: what the per-region-overlap (PRO) curve
// of the MVTec evaluation weights its pixels by.  The labelling is labeller.h's tiled union-find (tile pass, border merge,
// root sizes) with the one-class policy below: a pixel is defective or not, so "the neighbour is my own" is the sign of
// its link.  label_tile is a wrapper around its tile body; the other passes are this file's own:
//   merge_borders  a thread per pixel of a tile's first column / first row: united with its (up to 3) neighbours in
//                  the tile to the left / above by atomicMin on the global links.
//   root_sizes     every tile root finds its region root, adds its count there and links to it (unionfind.h).
//   finish_labels  every pixel: label = 1 + region root, size = the root's count; the totals {regions, defective, ok}.
// Labels and sizes are a function of the mask alone (labeller.h says why).
#include "labeller.h"

namespace {

using namespace uf;                                   // tiles, links, find_root (unionfind.h); the bodies (labeller.h)
constexpr int FIN_ITEMS = 8;                           // pixels per lane of finish_labels: 3 count atomics per 2048 pixels

struct LabelParams {
  const float* truth; const uint8_t* select;
  int h, w, tiles_x, tiles_y;
  long long per;                                       // h * w
  int* parent; int* labels; int* sizes;
  unsigned long long* counts;                          // {regions, defective, ok}
};

// labeller.h's pixel policy for image n: one class (defective); the images of `select` (NULL: all)
struct MaskPixels {
  const float* truth; const uint8_t* select;           // the image's plane; its entry of `select`, or NULL
  static constexpr bool BY_CLASS = false;
  __device__ __forceinline__ int cls(long long g) const { return truth[g] > 0.5f; }
  __device__ __forceinline__ bool selected() const { return !select || *select; }
};
__device__ __forceinline__ MaskPixels pixels_of(const LabelParams& A, int n) {
  return MaskPixels{A.truth + (long long)n * A.per, A.select ? A.select + n : nullptr};
}
__device__ __forceinline__ Frame frame_of(const LabelParams& A, int n) {
  return Frame{A.h, A.w, A.tiles_x, A.per, A.parent + (long long)n * A.per, A.sizes + (long long)n * A.per};
}

__global__ __launch_bounds__(LT_THREADS) void label_tile(const LabelParams A) {
  label_tile_body(pixels_of(A, blockIdx.y), frame_of(A, blockIdx.y));
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
  return launch_labeller<LabelParams>({label_tile, "label_tile"}, {merge_borders, "merge_borders"}, {root_sizes, "root_sizes"},
                                      {finish_labels, "finish_labels"}, A, n, h, w, FIN_ITEMS, s);
}
