// The tiled union-find labeller of 8-connected regions, shared by regions.hip (defective pixels of a float mask) and
// segregions.hip (pixels of one class of a uint8 label map); the links, find_root and unite are unionfind.h's.  Four
// launches, no workgroup waits on another:
//   tile pass     a 32x32 tile in LDS: every pixel with a class is united with its W neighbour and with N, or (N not its
//                 own) NW and NE, where they are its own, by atomicMin on the links; each pixel then finds its tile root.
//                 Writes the root's image index as the pixel's global link (-1: no class) and, at the root, the pixel count
//                 of the tile component.
//   border merge  a thread per pixel of a tile's first column / first row: united with those of its (up to 3) neighbours
//                 in the tile to the left / above that are its own, by atomicMin on the global links.
//   root sizes    every tile root finds its region root, adds its count there (integer atomicAdd) and links to it.
//   finish        the caller's own kernel: label = 1 + region root, size = the root's count, and what it counts.
// The tile pass is a template here, over a pixel policy P that the caller makes for the block's image, and the callers
// keep their __global__ kernels as wrappers around it:
//   int  P::cls(long long g) const   class of pixel g of the image; 0 = none, not labelled
//   bool P::selected() const         false: the image is left out
//   P::BY_CLASS                      how "the neighbour is my own" is tested.  false: there is one class, so any neighbour
//                                    with a link (>= 0) is; the sign of the link says so.  true: the neighbour's class is
//                                    compared, from a tile of classes in LDS.
// The launch sequence is here too.  The border merge, the root sizes and the finish pass stay in the callers: shared
// bodies changed the register counts of the merge and root-size kernels (profiles/shared_bodies.txt).
// A link only ever decreases and always stays inside its region, so a stale read costs a retry, never a wrong union; the
// minimum index of a region is its only possible root, so labels and sizes are a function of the input alone.
#pragma once
#include "unionfind.h"

namespace uf {

// The frame of the block's image: the wrappers fill it from their parameter structs
struct Frame {
  int h, w, tiles_x;
  long long per;                                       // h * w
  int* parent; int* sizes;                             // the image's planes
};

// grid (tiles of one image, images), LT_THREADS
template <class P>
__device__ __forceinline__ void label_tile_body(const P& px, const Frame& A) {
  __shared__ int par[LT_PIX];
  __shared__ int cnt[LT_PIX];
  uint8_t* kls = nullptr;                              // BY_CLASS: written once before the barrier, then only read
  if constexpr (P::BY_CLASS) {
    __shared__ uint8_t tile_classes[LT_PIX];
    kls = tile_classes;
  }
  if (!px.selected()) return;                          // block-uniform
  const int y0 = (int)(blockIdx.x / A.tiles_x) * LT, x0 = (int)(blockIdx.x % A.tiles_x) * LT;
  constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
  int c[LT_ITEMS];
#pragma unroll
  for (int j = 0; j < LT_ITEMS; ++j) {
    const int i = threadIdx.x + j * LT_THREADS, y = y0 + i / LT, x = x0 + i % LT;
    c[j] = (y < A.h && x < A.w) ? px.cls((long long)y * A.w + x) : 0;
    par[i] = c[j] ? i : -1;
    cnt[i] = 0;
    if constexpr (P::BY_CLASS) kls[i] = (uint8_t)c[j];
  }
  __syncthreads();
  // neighbour i2 of a pixel of class k is its own
  const auto own = [&](int i2, int k) {
    if constexpr (P::BY_CLASS) return kls[i2] == k;
    else return link_of<WG>(par, i2) >= 0;
  };
#pragma unroll
  for (int j = 0; j < LT_ITEMS; ++j) {
    if (!c[j]) continue;
    const int i = threadIdx.x + j * LT_THREADS, ly = i / LT, lx = i % LT;
    if (lx > 0 && own(i - 1, c[j])) unite<WG>(par, i, i - 1);
    if (ly > 0) {
      if (own(i - LT, c[j])) {                         // N joins NW and NE by their own W links
        unite<WG>(par, i, i - LT);
      } else {
        if (lx > 0 && own(i - LT - 1, c[j])) unite<WG>(par, i, i - LT - 1);
        if (lx < LT - 1 && own(i - LT + 1, c[j])) unite<WG>(par, i, i - LT + 1);
      }
    }
  }
  __syncthreads();
  int root[LT_ITEMS];
#pragma unroll
  for (int j = 0; j < LT_ITEMS; ++j) {
    root[j] = c[j] ? find_root<WG>(par, threadIdx.x + j * LT_THREADS) : -1;
    if (c[j]) atomicAdd(&cnt[root[j]], 1);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < LT_ITEMS; ++j) {
    const int i = threadIdx.x + j * LT_THREADS, y = y0 + i / LT, x = x0 + i % LT;
    if (y >= A.h || x >= A.w) continue;
    const long long g = (long long)y * A.w + x;
    // the tile's row-major order follows the image's: the tile root is the component's smallest image index too
    A.parent[g] = c[j] ? (y0 + root[j] / LT) * A.w + x0 + root[j] % LT : -1;
    A.sizes[g] = root[j] == i ? cnt[i] : 0;
  }
}

// A kernel of the launch sequence and the name its launch is checked under
template <class Params>
struct Pass {
  void (*kernel)(const Params);
  const char* name;
};

// The launch sequence for n images of h x w: the tile pass, the border merge and the root sizes when there is a border
// (one tile: every tile root is a region root already), then the caller's finish kernel with fin_items pixels per lane.
template <class Params>
int32_t launch_labeller(Pass<Params> tile, Pass<Params> merge, Pass<Params> sizes, Pass<Params> finish, const Params& A,
                        int64_t n, int64_t h, int64_t w, int fin_items, hipStream_t s) {
  const long long tx = cdiv64(w, LT), ty = cdiv64(h, LT), border = (tx - 1) * h + (ty - 1) * w;
  const auto run = [&](const Pass<Params>& p, long long blocks, int threads) {
    hipLaunchKernelGGL(p.kernel, dim3((unsigned)blocks, (unsigned)n), dim3(threads), 0, s, A);
    return unet_check_launch(p.name);
  };
  int32_t rc = run(tile, tx * ty, LT_THREADS);
  if (rc == UNET_OK && border > 0) rc = run(merge, cdiv64(border, PX_THREADS), PX_THREADS);
  if (rc == UNET_OK && border > 0) rc = run(sizes, cdiv64(h * w, PX_THREADS), PX_THREADS);
  if (rc == UNET_OK) rc = run(finish, cdiv64(h * w, (long long)PX_THREADS * fin_items), PX_THREADS);
  return rc;
}

}  // namespace uf
