// Groups of class regions: the fragments of one defect that a prediction broke apart, joined again.  classes, region
// and sizes are what unet_label_class_regions takes and makes.  A fragment is a region with size >= min_pixels; smaller
// regions are dropped first, so they link nothing and join nothing.  Two fragments of one image and one class are linked
// iff they hold pixels p, q with (py - qy)^2 + (px - qx)^2 <= gap^2, and a group is a connected component of the link
// graph: linking is transitive.  Four launches over a per-pixel link plane and a per-pixel count plane in the workspace,
// integers only, no workgroup waits on another:
//   init_fragment_links    every pixel: a fragment root (region == own index + 1, kept) links to itself, every other
//                          pixel gets -1; the count plane is cleared.
//   link_fragment_tile     a 32x32 tile with its halo in LDS (one row above, gap rows below, gap columns each side):
//                          the kept region id (0: background, dropped, outside the frame) and the class of every cell.
//                          Only edge pixels search: a pixel with a 4-neighbour inside the frame that is not of its
//                          region.  A closest pair of two regions has both ends on such pixels (a pixel whose in-frame
//                          4-neighbours are all its own could step towards the other end and stay in its region).  An
//                          edge pixel scans the half-disc dy > 0, or dy == 0 and dx > 0, so every pair is met from its
//                          row-major first pixel; where the cell has its class and another id, the two fragment roots are
//                          united on the global links (unionfind.h) and then linked straight to the root found, so
//                          that the many later hits on the same pair cost one load.  The halo is addressed by (row,
//                          column), so a row never wraps into the next.
//   resolve_fragments      every fragment root finds its group root, adds its size to the group root's count, links to
//                          it, appends its record and, if it is the group root, counts the group for its class.
//   finish_groups          every pixel of a fragment: group = 1 + its fragment root's group root, group_sizes = that
//                          root's count; 0 elsewhere.
// Termination and determinism are unionfind.h's: links only fall and stay inside their group, nobody waits, and the
// smallest fragment root of a group is its only possible root, so every output but the record order is a function of
// the inputs alone.  Ids are checked against the frame before they index anything: maps that do not belong together give
// wrong groups, never an access outside the planes.
#include "segpixel.h"
#include "slots.h"

namespace {

using namespace uf;
using segpx::class_of;
using slots::wave_slot;
constexpr int MAX_GAP = 32;
constexpr int HALO_H = LT + 1 + MAX_GAP;               // one row above, gap rows below
constexpr int HALO_W = LT + 2 * MAX_GAP;               // gap columns each side
constexpr int FIN_ITEMS = 4;                           // pixels per lane of the per-pixel passes
constexpr int FREC = 5;                                // int64 fields of a fragment record
constexpr int DEV = __HIP_MEMORY_SCOPE_AGENT;
static_assert(PX_THREADS == 256 && LT_THREADS == 256, "one class counter per thread; four tile pixels per thread");

struct GroupParams {
  const uint8_t* cls; const int* region; const int* sizes;
  int C, h, w, tiles_x, gap, min_pixels, image_base;
  long long per;                                       // h * w
  int* link; int* gcount;                              // [n][h][w] workspace planes
  int* group; int* group_sizes;
  unsigned long long* counts;                          // [n][C] groups per image and class
  long long* fragments; long long capacity;
  unsigned long long* fragment_count;
};

// the id of pixel g's region if that region is a fragment (kept, and an id of this frame), else 0
__device__ __forceinline__ int kept_id(const GroupParams& A, long long base, long long g) {
  const int id = A.region[base + g];
  return (id > 0 && id <= A.per && A.sizes[base + g] >= A.min_pixels) ? id : 0;
}

// grid (pixels of one image / (PX_THREADS * FIN_ITEMS), images)
__global__ __launch_bounds__(PX_THREADS) void init_fragment_links(const GroupParams A) {
  const long long base = (long long)blockIdx.y * A.per;
#pragma unroll
  for (int k = 0; k < FIN_ITEMS; ++k) {
    const long long g = ((long long)blockIdx.x * FIN_ITEMS + k) * PX_THREADS + threadIdx.x;
    if (g >= A.per) break;
    A.link[base + g] = kept_id(A, base, g) == (int)g + 1 ? (int)g : -1;
    A.gcount[base + g] = 0;
  }
}

// grid (tiles of one image, images), LT_THREADS
__global__ __launch_bounds__(LT_THREADS) void link_fragment_tile(const GroupParams A) {
  __shared__ int ids[HALO_H * HALO_W];                 // written once before the barrier, then only read
  __shared__ uint8_t kls[HALO_H * HALO_W];
  const long long base = (long long)blockIdx.y * A.per;
  const int y0 = (int)(blockIdx.x / A.tiles_x) * LT, x0 = (int)(blockIdx.x % A.tiles_x) * LT;
  const int gap = A.gap, sw = LT + 2 * gap, sh = LT + 1 + gap;      // the halo in use: rows y0 - 1 .., columns x0 - gap ..
  for (int i = threadIdx.x; i < sh * sw; i += LT_THREADS) {
    const int y = y0 - 1 + i / sw, x = x0 - gap + i % sw;
    int id = 0, c = 0;
    if (y >= 0 && y < A.h && x >= 0 && x < A.w) {
      const long long g = (long long)y * A.w + x;
      id = kept_id(A, base, g);
      c = id ? class_of(A.cls[base + g], A.C) : 0;
    }
    ids[i] = c ? id : 0;
    kls[i] = (uint8_t)c;
  }
  __syncthreads();
  int* link = A.link + base;
  const int gap_sq = gap * gap;
#pragma unroll 1
  for (int j = 0; j < LT_ITEMS; ++j) {
    const int i = threadIdx.x + j * LT_THREADS, ly = i / LT, lx = i % LT;
    const int y = y0 + ly, x = x0 + lx;
    const int s = (ly + 1) * sw + lx + gap;            // the pixel's cell
    const int id = ids[s];
    if (!id) continue;                                 // no fragment here (or outside the frame)
    const int c = kls[s];
    // a cell outside the frame holds 0 and must not make an edge pixel: the frame is tested first
    const bool edge = (y > 0 && ids[s - sw] != id) || (y < A.h - 1 && ids[s + sw] != id) ||
                      (x > 0 && ids[s - 1] != id) || (x < A.w - 1 && ids[s + 1] != id);
    if (!edge) continue;
    int last = id;                                     // the id this pixel united with last: most cells repeat it
    int mine = -1;                                     // a member of this fragment's group: its root when last looked up
    int lim = gap;                                     // the largest |dx| with dy^2 + dx^2 <= gap^2
    for (int dy = 0; dy <= gap; ++dy) {
      while (lim * lim + dy * dy > gap_sq) --lim;
      const int row = s + dy * sw;
      for (int dx = dy ? -lim : 1; dx <= lim; ++dx) {
        const int q = ids[row + dx];
        if (q == 0 || q == id || q == last || kls[row + dx] != c) continue;
        last = q;
        // both are fragment roots of this frame unless the maps do not belong together
        const int lq = link_of<DEV>(link, q - 1);
        if (lq < 0 || link_of<DEV>(link, id - 1) < 0) continue;
        if (mine < 0) mine = find_root<DEV>(link, id - 1);
        if (lq == mine) continue;                      // q hangs below a member of my group: one load, the common case
        unite<DEV>(link, id - 1, q - 1);
        // both fragments then link to the root found: it is of their group and not above them (a root is its group's
        // smallest index), so the links only fall, and the next pixel that meets the pair takes the short way above
        mine = find_root<DEV>(link, id - 1);
        atomicMin(&link[id - 1], mine);
        atomicMin(&link[q - 1], mine);
      }
    }
  }
}

// grid (pixels of one image / (PX_THREADS * FIN_ITEMS), images); every lane runs every round (the ballots want that)
__global__ __launch_bounds__(PX_THREADS) void resolve_fragments(const GroupParams A) {
  __shared__ unsigned int roots[256];                  // group roots of this block, by class
  const int n = blockIdx.y;
  const long long base = (long long)n * A.per;
  const int lane = threadIdx.x & (WAVE - 1);
  int* link = A.link + base;
  roots[threadIdx.x] = 0u;                             // PX_THREADS == 256 >= C
  __syncthreads();
#pragma unroll
  for (int k = 0; k < FIN_ITEMS; ++k) {
    const long long g = ((long long)blockIdx.x * FIN_ITEMS + k) * PX_THREADS + threadIdx.x;
    const bool frag = g < A.per && link_of<DEV>(link, (int)g) >= 0;
    const long long slot = wave_slot(A.fragment_count, frag, lane);
    if (!frag) continue;
    const int r = find_root<DEV>(link, (int)g);        // final: every union was made by the launch before
    const int size = A.sizes[base + g], c = class_of(A.cls[base + g], A.C);
    atomicAdd(&A.gcount[base + r], size);              // integer: exact in any order
    if (r == (int)g) atomicAdd(&roots[c], 1u);
    else __hip_atomic_store(&link[g], r, __ATOMIC_RELAXED, DEV);      // still a pixel of its group, and below
    if (slot < A.capacity) {                           // a record past the capacity is counted and not written
      long long* rec = A.fragments + slot * FREC;
      rec[0] = (long long)A.image_base + n; rec[1] = c; rec[2] = g; rec[3] = r; rec[4] = size;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x > 0 && (int)threadIdx.x < A.C && roots[threadIdx.x])
    atomicAdd(&A.counts[(long long)n * A.C + threadIdx.x], (unsigned long long)roots[threadIdx.x]);
}

// same grid as resolve_fragments, after it
__global__ __launch_bounds__(PX_THREADS) void finish_groups(const GroupParams A) {
  const long long base = (long long)blockIdx.y * A.per;
  const int* link = A.link + base;
#pragma unroll
  for (int k = 0; k < FIN_ITEMS; ++k) {
    const long long g = ((long long)blockIdx.x * FIN_ITEMS + k) * PX_THREADS + threadIdx.x;
    if (g >= A.per) break;
    int label = 0, size = 0;
    const int id = kept_id(A, base, g);
    if (id && link[id - 1] >= 0) {
      const int r = find_root<DEV>(link, id - 1);      // at most fragment root -> group root
      label = r + 1;
      size = A.gcount[base + r];
    }
    A.group[base + g] = label;
    A.group_sizes[base + g] = size;
  }
}

inline bool supported(int64_t n, int64_t h, int64_t w, int64_t C) {
  return frames_supported(n, h, w) && C >= 2 && C <= 255;
}

}  // namespace

extern "C" size_t unet_group_class_regions_workspace(int64_t n, int64_t h, int64_t w, int32_t num_classes) {
  if (!supported(n, h, w, num_classes)) return 0;
  return up16((size_t)(n * h * w) * 8);
}

extern "C" int32_t unet_group_class_regions(const uint8_t* classes, const int32_t* region, const int32_t* sizes,
                                            int64_t n, int64_t h, int64_t w, int32_t num_classes, int32_t gap,
                                            int32_t min_pixels, int32_t image_base, int32_t* group,
                                            int32_t* group_sizes, int64_t* counts, int64_t* fragments, int64_t capacity,
                                            int64_t* fragment_count, void* workspace, size_t workspace_bytes,
                                            void* stream) {
  UNET_REQUIRE(classes && region && sizes && group && group_sizes && counts && fragments && fragment_count && workspace,
               UNET_ERR_BAD_ARG, "unet_group_class_regions: null pointer");
  UNET_REQUIRE(n > 0 && h > 0 && w > 0 && gap >= 1 && gap <= MAX_GAP && min_pixels >= 1 && image_base >= 0 &&
                   capacity >= 0,
               UNET_ERR_BAD_ARG, "unet_group_class_regions: n=%lld h=%lld w=%lld gap=%d (1..32) min_pixels=%d "
               "image_base=%d capacity=%lld", (long long)n, (long long)h, (long long)w, (int)gap, (int)min_pixels,
               (int)image_base, (long long)capacity);
  UNET_REQUIRE(supported(n, h, w, num_classes) && (int64_t)image_base + n <= (1LL << 31) - 1, UNET_ERR_UNSUPPORTED,
               "unet_group_class_regions: n=%lld h=%lld w=%lld classes=%d (n < 65536, at most 2^31 - 1 pixels, 2..255 "
               "classes, image indices below 2^31)", (long long)n, (long long)h, (long long)w, (int)num_classes);
  UNET_REQUIRE(workspace_bytes >= unet_group_class_regions_workspace(n, h, w, num_classes), UNET_ERR_WORKSPACE,
               "unet_group_class_regions: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const long long pixels = (long long)(n * h * w);
  const int tx = (int)cdiv64(w, LT), ty = (int)cdiv64(h, LT);
  GroupParams A{classes, region, sizes, (int)num_classes, (int)h, (int)w, tx, (int)gap, (int)min_pixels, (int)image_base,
                (long long)(h * w), (int*)workspace, (int*)workspace + pixels, group, group_sizes,
                (unsigned long long*)counts, (long long*)fragments, (long long)capacity,
                (unsigned long long*)fragment_count};
  ProfScope prof(UNET_K_OTHER, 0.0, s, "link_fragment_tile", (double)pixels * 33.0);
  const dim3 px((unsigned)cdiv64(h * w, PX_THREADS * FIN_ITEMS), (unsigned)n);
  hipLaunchKernelGGL(init_fragment_links, px, dim3(PX_THREADS), 0, s, A);
  int32_t rc = unet_check_launch("init_fragment_links");
  if (rc) return rc;
  hipLaunchKernelGGL(link_fragment_tile, dim3((unsigned)((long long)tx * ty), (unsigned)n), dim3(LT_THREADS), 0, s, A);
  rc = unet_check_launch("link_fragment_tile");
  if (rc) return rc;
  hipLaunchKernelGGL(resolve_fragments, px, dim3(PX_THREADS), 0, s, A);
  rc = unet_check_launch("resolve_fragments");
  if (rc) return rc;
  hipLaunchKernelGGL(finish_groups, px, dim3(PX_THREADS), 0, s, A);
  return unet_check_launch("finish_groups");
}
