// Union-find on parent links, shared by the region labellers (regions.hip: defective pixels; segregions.hip: pixels of
// one class).  A link is the index of a pixel of the same region with a smaller or equal index; a root links to itself.
// Why every loop here ends: links are only ever lowered (atomicMin, or a store of the found root, which is below), never
// below 0, and only to an index of the same region.  find_root follows strictly decreasing indices, so it ends at a
// root.  unite retries only when its atomicMin found the link already lowered by somebody else; the links of a tile or
// an image can be lowered finitely often, so the retries are finite whatever the other threads do, and no thread ever
// waits for another.  A stale read costs a retry, never a wrong union.
#pragma once
#include "common.h"

namespace uf {

constexpr int LT = 32;                                 // tile edge
constexpr int LT_PIX = LT * LT;
constexpr int LT_THREADS = 256;
constexpr int LT_ITEMS = LT_PIX / LT_THREADS;
constexpr int PX_THREADS = 256;

template <int SCOPE>
__device__ __forceinline__ int link_of(const int* L, int i) { return __hip_atomic_load(&L[i], __ATOMIC_RELAXED, SCOPE); }

template <int SCOPE>
__device__ __forceinline__ int find_root(const int* L, int i) {
  int r = link_of<SCOPE>(L, i);
  while (r != i) { i = r; r = link_of<SCOPE>(L, i); }
  return r;
}

// the larger root is linked below the smaller; a lost race (the link was no longer a's own) carries on from what
// the atomic returned, which is in a's set
template <int SCOPE>
__device__ __forceinline__ void unite(int* L, int a, int b) {
  for (;;) {
    a = find_root<SCOPE>(L, a);
    b = find_root<SCOPE>(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&L[a], b);
    if (old == a) return;
    a = old;
  }
}

// Pixel g of one image after the border merge: a tile root (sizes[g] > 0: the pixel count of its tile component) finds
// its region root, adds its count there (integer atomicAdd) and links to it.  Only region roots are added to and only
// they are read by other threads (sign only: a tile root's count is positive from the start), so the adds need no
// second array.
__device__ __forceinline__ void add_tile_root(int* parent, int* sizes, int g) {
  const int own = __hip_atomic_load(&sizes[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (own <= 0) return;                                // not a tile root
  const int r = find_root<__HIP_MEMORY_SCOPE_AGENT>(parent, g);
  if (r == g) return;
  atomicAdd(&sizes[r], own);                           // integer: exact in any order; nobody adds to a non-root
  __hip_atomic_store(&parent[g], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// n < 65536 images (grid y) and at most 2^31 - 1 pixels in all (int32 links and labels)
inline bool frames_supported(int64_t n, int64_t h, int64_t w) {
  if (n <= 0 || h <= 0 || w <= 0 || n >= 65536) return false;
  const int64_t lim = (1LL << 31) - 1;
  if (h > lim || w > lim || h > lim / w) return false;
  return n <= lim / (h * w);                           // n h w <= 2^31 - 1
}
inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

}  // namespace uf
