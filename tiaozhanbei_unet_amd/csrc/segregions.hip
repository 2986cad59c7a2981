// Class regions of uint8 label maps and how much of each the other map covers: the defect-level counterpart of the
// pixel statistics of segeval.hip.  A pixel has class c iff its value is c with 1 <= c < C (0 and every value >= C are
// background); a class region is an 8-connected component of pixels of one and the same class in one image.
//
// Labelling is labeller.h's tiled union-find (label_class_tile is a wrapper around its tile body) with
// the by-class policy below: "the neighbour is my own" means "the neighbour has my class".  This file's own passes:
//   merge_class_borders   a thread per pixel of a tile's first column / first row: united with those of its (up to 3)
//                         neighbours in the tile to the left / above that have its class.
//   class_root_sizes      every tile root adds its count at its region root and links to it (unionfind.h).
//   finish_class_regions  every pixel: region = 1 + region root, size = the root's count; regions per image and class.
// Matching is two more launches over the pixels, integers only:
//   count_class_hits      a pixel whose truth and predicted class agree (not background) and whose predicted region is
//                         kept (size >= min_pixels) adds 1 at the root pixel of its truth region and at the root pixel of
//                         its predicted region: one atomicAdd per wave and root where the lanes share the root.
//   emit_class_records    every root pixel of a truth region / of a kept predicted region appends (image, class, root
//                         index, size, hit) to its record buffer; the slot comes from one atomicAdd per wave on the
//                         device-side count, so the order is arbitrary and the caller sorts by (image, root index).
// Termination: the only loops that are not counted are find_root and unite (unionfind.h).  A link is only ever lowered,
// never below 0, and only to a pixel that has been united with its owner, and unions are only made between neighbours of
// one class: every link stays inside its class region, every chain descends to a root, and the retries of unite are
// bounded by the finitely many times the links can be lowered.  The smallest index of a region is its only possible
// root, so every output but the record order is a function of the two label maps alone.
#include "labeller.h"
#include "segpixel.h"
#include "slots.h"

namespace {

using namespace uf;                                   // tiles, links, find_root (unionfind.h); the bodies (labeller.h)
using segpx::class_of;
using slots::wave_slot;
constexpr int FIN_ITEMS = 8;                           // pixels per lane of the per-pixel passes
constexpr int REC = 5;                                 // int32 fields of a record
static_assert(PX_THREADS == 256, "finish_class_regions keeps one counter per thread and class");

struct ClassParams {
  const uint8_t* cls; int C;
  int h, w, tiles_x, tiles_y;
  long long per;                                       // h * w
  int* parent; int* region; int* sizes;
  unsigned long long* counts;                          // [n][C] regions per image and class
};

// labeller.h's pixel policy for image n: the classes 1 .. C - 1 of a label map, every image
struct ClassPixels {
  const uint8_t* map; int C;                           // the image's plane
  static constexpr bool BY_CLASS = true;
  __device__ __forceinline__ int cls(long long g) const { return class_of(map[g], C); }
  __device__ __forceinline__ bool selected() const { return true; }
};
__device__ __forceinline__ ClassPixels pixels_of(const ClassParams& A, int n) {
  return ClassPixels{A.cls + (long long)n * A.per, A.C};
}
__device__ __forceinline__ Frame frame_of(const ClassParams& A, int n) {
  return Frame{A.h, A.w, A.tiles_x, A.per, A.parent + (long long)n * A.per, A.sizes + (long long)n * A.per};
}

__global__ __launch_bounds__(LT_THREADS) void label_class_tile(const ClassParams A) {
  label_tile_body(pixels_of(A, blockIdx.y), frame_of(A, blockIdx.y));
}

// grid (border pixels of one image / PX_THREADS, images): first the (tiles_x - 1) * h pixels of the tiles' first
// columns, then the (tiles_y - 1) * w pixels of their first rows.  Two pixels of different tiles that touch differ in
// their tile row (the lower one is in a first row, the other one row above and at most one column away) or only in
// their tile column (the right one is in a first column, the other one column to the left): every such pair is seen.
__global__ __launch_bounds__(PX_THREADS) void merge_class_borders(const ClassParams A) {
  const int n = blockIdx.y;
  constexpr int DEV = __HIP_MEMORY_SCOPE_AGENT;
  const long long cols = (long long)(A.tiles_x - 1) * A.h, rows = (long long)(A.tiles_y - 1) * A.w;
  long long b = (long long)blockIdx.x * PX_THREADS + threadIdx.x;
  if (b >= cols + rows) return;
  int* parent = A.parent + (long long)n * A.per;
  const uint8_t* t = A.cls + (long long)n * A.per;
  int x, y, dx, dy;                                    // the neighbours are (x - 1 + k dx, y - 1 + k dy), k = 0, 1, 2
  if (b < cols) {
    x = (int)(b / A.h + 1) * LT; y = (int)(b % A.h); dx = 0; dy = 1;
  } else {
    b -= cols;
    y = (int)(b / A.w + 1) * LT; x = (int)(b % A.w); dx = 1; dy = 0;
  }
  const int p = y * A.w + x;
  const int c = class_of(t[p], A.C);
  if (!c) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int qx = x - 1 + k * dx, qy = y - 1 + k * dy;
    if (qx < 0 || qy < 0 || qx >= A.w || qy >= A.h) continue;
    const int q = qy * A.w + qx;
    if (class_of(t[q], A.C) == c) unite<DEV>(parent, p, q);
  }
}

// grid (pixels of one image / PX_THREADS, images)
__global__ __launch_bounds__(PX_THREADS) void class_root_sizes(const ClassParams A) {
  const long long g = (long long)blockIdx.x * PX_THREADS + threadIdx.x;
  if (g >= A.per) return;
  const long long base = (long long)blockIdx.y * A.per;
  add_tile_root(A.parent + base, A.sizes + base, (int)g);
}

// grid (pixels of one image / (PX_THREADS * FIN_ITEMS), images)
__global__ __launch_bounds__(PX_THREADS) void finish_class_regions(const ClassParams A) {
  __shared__ unsigned int roots[256];                  // region roots of this block, by class
  const int n = blockIdx.y;
  const long long base = (long long)n * A.per;
  const int* parent = A.parent + base;
  roots[threadIdx.x] = 0u;                             // PX_THREADS == 256 >= C
  __syncthreads();
#pragma unroll
  for (int k = 0; k < FIN_ITEMS; ++k) {
    const long long g = ((long long)blockIdx.x * FIN_ITEMS + k) * PX_THREADS + threadIdx.x;
    if (g >= A.per) break;
    int label = 0, size = 0;
    if (parent[g] >= 0) {
      const int r = find_root<__HIP_MEMORY_SCOPE_AGENT>(parent, (int)g);     // at most tile root -> region root
      label = r + 1;
      size = A.sizes[base + r];                        // a root's entry is never written here
      if (r == (int)g) atomicAdd(&roots[class_of(A.cls[base + g], A.C)], 1u);
    }
    A.region[base + g] = label;
    if (label != (int)g + 1) A.sizes[base + g] = size;
  }
  __syncthreads();
  if ((int)threadIdx.x < A.C && roots[threadIdx.x])
    atomicAdd(&A.counts[(long long)n * A.C + threadIdx.x], (unsigned long long)roots[threadIdx.x]);
}

struct MatchParams {
  const uint8_t* tcls; const int* treg; const int* tsz;
  const uint8_t* pcls; const int* preg; const int* psz;
  int C, min_pixels, image_base;
  long long per;
  int* thit; int* phit;                                // [n][h][w], zeroed; only the root pixels are added to
  int* trec; int* prec; long long capacity;
  unsigned long long* rec_counts;                      // {truth records, predicted records}
};

// hits[root] += 1 for every lane that is on: the lanes that share the root of the first such lane (a whole wave inside
// one region) add their number once, the others one each
__device__ __forceinline__ void wave_add(int* hits, int root, bool on, int lane) {
  const unsigned long long m = __ballot(on);
  if (!m) return;                                      // wave-uniform
  const int lead = __shfl(root, __ffsll((long long)m) - 1);
  const unsigned long long same = __ballot(on && root == lead);
  if (!on) return;
  if (root != lead) atomicAdd(&hits[root], 1);
  else if (!(same & ((1ull << lane) - 1ull))) atomicAdd(&hits[lead], (int)__popcll(same));
}

// grid (pixels of one image / (PX_THREADS * FIN_ITEMS), images); every lane runs every round (the ballots want that)
__global__ __launch_bounds__(PX_THREADS) void count_class_hits(const MatchParams A) {
  const long long base = (long long)blockIdx.y * A.per;
  const int lane = threadIdx.x & (WAVE - 1);
#pragma unroll
  for (int k = 0; k < FIN_ITEMS; ++k) {
    const long long g = ((long long)blockIdx.x * FIN_ITEMS + k) * PX_THREADS + threadIdx.x;
    bool hit = false;
    int tr = 0, pr = 0;
    if (g < A.per) {
      const int tc = class_of(A.tcls[base + g], A.C);
      if (tc && class_of(A.pcls[base + g], A.C) == tc && A.psz[base + g] >= A.min_pixels) {
        tr = A.treg[base + g] - 1;                     // class pixels have a region: 0 <= root < per; maps that
        pr = A.preg[base + g] - 1;                     // do not belong to the regions must not write elsewhere
        hit = tr >= 0 && tr < A.per && pr >= 0 && pr < A.per;
      }
    }
    wave_add(A.thit + base, tr, hit, lane);
    wave_add(A.phit + base, pr, hit, lane);
  }
}

__device__ __forceinline__ void put_record(int* rec, long long slot, long long capacity, int image, int cls, int root,
                                           int size, int hit) {
  if (slot < 0 || slot >= capacity) return;            // counted but not kept: the caller sees count > capacity
  int* r = rec + slot * REC;
  r[0] = image; r[1] = cls; r[2] = root; r[3] = size; r[4] = hit;
}

// same grid as count_class_hits, after it
__global__ __launch_bounds__(PX_THREADS) void emit_class_records(const MatchParams A) {
  const int n = blockIdx.y;
  const long long base = (long long)n * A.per;
  const int lane = threadIdx.x & (WAVE - 1);
#pragma unroll
  for (int k = 0; k < FIN_ITEMS; ++k) {
    const long long g = ((long long)blockIdx.x * FIN_ITEMS + k) * PX_THREADS + threadIdx.x;
    const bool in = g < A.per;
    const bool troot = in && A.treg[base + g] == (int)g + 1;
    const int psize = in ? A.psz[base + g] : 0;
    const bool proot = in && A.preg[base + g] == (int)g + 1 && psize >= A.min_pixels;
    const long long ts = wave_slot(&A.rec_counts[0], troot, lane);
    const long long ps = wave_slot(&A.rec_counts[1], proot, lane);
    if (troot)
      put_record(A.trec, ts, A.capacity, A.image_base + n, class_of(A.tcls[base + g], A.C), (int)g, A.tsz[base + g],
                 A.thit[base + g]);
    if (proot)
      put_record(A.prec, ps, A.capacity, A.image_base + n, class_of(A.pcls[base + g], A.C), (int)g, psize,
                 A.phit[base + g]);
  }
}

inline bool supported(int64_t n, int64_t h, int64_t w, int64_t C) {
  return frames_supported(n, h, w) && C >= 2 && C <= 255;
}

}  // namespace

extern "C" size_t unet_label_class_regions_workspace(int64_t n, int64_t h, int64_t w, int32_t num_classes) {
  if (!supported(n, h, w, num_classes)) return 0;
  return up16((size_t)(n * h * w) * 4);
}

extern "C" int32_t unet_label_class_regions(const uint8_t* classes, int64_t n, int64_t h, int64_t w, int32_t num_classes,
                                            int32_t* region, int32_t* sizes, int64_t* counts, void* workspace,
                                            size_t workspace_bytes, void* stream) {
  UNET_REQUIRE(classes && region && sizes && counts && workspace, UNET_ERR_BAD_ARG,
               "unet_label_class_regions: null pointer");
  UNET_REQUIRE(n > 0 && h > 0 && w > 0, UNET_ERR_BAD_ARG, "unet_label_class_regions: n=%lld h=%lld w=%lld", (long long)n,
               (long long)h, (long long)w);
  UNET_REQUIRE(supported(n, h, w, num_classes), UNET_ERR_UNSUPPORTED,
               "unet_label_class_regions: n=%lld h=%lld w=%lld classes=%d (n < 65536, at most 2^31 - 1 pixels, 2..255 "
               "classes)", (long long)n, (long long)h, (long long)w, (int)num_classes);
  UNET_REQUIRE(workspace_bytes >= unet_label_class_regions_workspace(n, h, w, num_classes), UNET_ERR_WORKSPACE,
               "unet_label_class_regions: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int tx = (int)cdiv64(w, LT), ty = (int)cdiv64(h, LT);
  ClassParams A{classes, (int)num_classes, (int)h, (int)w, tx, ty, (long long)(h * w), (int*)workspace, region, sizes,
                (unsigned long long*)counts};
  ProfScope prof(UNET_K_OTHER, 0.0, s, "label_class_tile", (double)n * h * w * 13.0);
  return launch_labeller<ClassParams>({label_class_tile, "label_class_tile"}, {merge_class_borders, "merge_class_borders"},
                                      {class_root_sizes, "class_root_sizes"},
                                      {finish_class_regions, "finish_class_regions"}, A, n, h, w, FIN_ITEMS, s);
}

extern "C" size_t unet_match_class_regions_workspace(int64_t n, int64_t h, int64_t w, int32_t num_classes) {
  if (!supported(n, h, w, num_classes)) return 0;
  return up16((size_t)(n * h * w) * 8);
}

extern "C" int32_t unet_match_class_regions(const uint8_t* truth, const int32_t* truth_region, const int32_t* truth_sizes,
                                            const uint8_t* pred, const int32_t* pred_region, const int32_t* pred_sizes,
                                            int64_t n, int64_t h, int64_t w, int32_t num_classes, int32_t min_pixels,
                                            int32_t image_base, int32_t* truth_records, int32_t* pred_records,
                                            int64_t capacity, int64_t* record_counts, void* workspace,
                                            size_t workspace_bytes, void* stream) {
  UNET_REQUIRE(truth && truth_region && truth_sizes && pred && pred_region && pred_sizes && truth_records &&
                   pred_records && record_counts && workspace,
               UNET_ERR_BAD_ARG, "unet_match_class_regions: null pointer");
  UNET_REQUIRE(n > 0 && h > 0 && w > 0 && min_pixels >= 1 && image_base >= 0 && capacity >= 0, UNET_ERR_BAD_ARG,
               "unet_match_class_regions: n=%lld h=%lld w=%lld min_pixels=%d image_base=%d capacity=%lld", (long long)n,
               (long long)h, (long long)w, (int)min_pixels, (int)image_base, (long long)capacity);
  UNET_REQUIRE(supported(n, h, w, num_classes) && (int64_t)image_base + n <= (1LL << 31) - 1, UNET_ERR_UNSUPPORTED,
               "unet_match_class_regions: n=%lld h=%lld w=%lld classes=%d (n < 65536, at most 2^31 - 1 pixels, 2..255 "
               "classes, image indices below 2^31)", (long long)n, (long long)h, (long long)w, (int)num_classes);
  const size_t need = unet_match_class_regions_workspace(n, h, w, num_classes);
  UNET_REQUIRE(workspace_bytes >= need, UNET_ERR_WORKSPACE, "unet_match_class_regions: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const long long pixels = (long long)(n * h * w);
  UNET_REQUIRE(hipMemsetAsync(workspace, 0, (size_t)pixels * 8, s) == hipSuccess, UNET_ERR_LAUNCH,
               "unet_match_class_regions: memset failed");
  MatchParams A{truth, truth_region, truth_sizes, pred, pred_region, pred_sizes, (int)num_classes, (int)min_pixels,
                (int)image_base, (long long)(h * w), (int*)workspace, (int*)workspace + pixels, truth_records,
                pred_records, (long long)capacity, (unsigned long long*)record_counts};
  ProfScope prof(UNET_K_OTHER, 0.0, s, "count_class_hits", (double)pixels * 36.0);
  const dim3 grid((unsigned)cdiv64(h * w, PX_THREADS * FIN_ITEMS), (unsigned)n);
  hipLaunchKernelGGL(count_class_hits, grid, dim3(PX_THREADS), 0, s, A);
  int32_t rc = unet_check_launch("count_class_hits");
  if (rc) return rc;
  hipLaunchKernelGGL(emit_class_records, grid, dim3(PX_THREADS), 0, s, A);
  return unet_check_launch("emit_class_records");
}
