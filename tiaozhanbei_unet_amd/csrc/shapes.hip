// Shape records of labelled class regions: second moments, bit-quad counts (Gray 1971) and the extent along D fixed
// directions of every region of unet_label_class_regions.  defects.hip says where a region lies and how sure the model
// was; this says how long, how wide, how round and how holed it is.  The host turns the integers into lengths
// (defects.shape_measures).
//
// A record is 11 + 2 D int64: image, root index, size, sum_xx, sum_yy, sum_xy, q1, q2, qd, q3, q4, pmin_0 .. pmin_{D-1},
// pmax_0 .. pmax_{D-1}.  Per member pixel (x, y) of the region, in raw frame coordinates and integers only:
//   moments      x x, y y, x y, summed.
//   bit quads    a 2 x 2 window of the region's own mask (everything else, the outside of the frame included, is a
//                non-member) is counted ONCE, by its first member in the order top-left, top-right, bottom-left,
//                bottom-right: that pixel sees the whole window among its 8 neighbours and knows the pattern (one member,
//                two edge-adjacent, two diagonal, three, four).  Every window with a member has exactly one first member,
//                so the counters are the per-window counts and no pixel reads another region's state.  Two pixels of one
//                class in one window touch at least by a corner, so they share a region: membership is region[] equality.
//   projections  p_k = x c_k + y s_k for the D direction vectors of the launch arguments; the record keeps min and max.
//                Only a pixel with a non-member among its 8 neighbours can be extreme (an interior pixel lies between two
//                members along every direction), so the others skip this part.
// Two launches over the pixels:
//   assign_shape_slots   defects.hip's assign pass: every root pixel of a kept region (size >= min_pixels) takes a slot,
//                        one atomicAdd per block on the device-side count, and writes its record as the region of that
//                        one pixel; every pixel leaves its slot or -1 in the 4-byte-per-pixel workspace, all of which is
//                        written.
//   accumulate_shapes    every other class pixel finds its slot at the root.  Moments and quads take defects.hip's way
//                        into the record: summed in the thread while the slot stays the same, then slots.h's
//                        flush_by_slot (across the wave for up to LEADERS slots, across the block through LDS), then int64
//                        atomicAdd at agent scope.  Projections:
//                        a lane takes the extremes of its own boundary pixels, the lanes of a wave that share the
//                        leading slot are reduced with shuffles, LEADERS times over, one direction after the other (no
//                        D values per lane in registers), and a lane on its own broadcasts its pixels; the commit has
//                        the lanes as directions, 2 D cells in one step.  A commit reads the
//                        record's value first and issues atomicMin / atomicMax only where it improves on it: a minimum
//                        only ever falls, so a value read earlier can only be too high and the skip is always right.
//                        That read is what a block-level fold would save, without D LDS cells per slot.
// No floating point: apart from the record order every output is a function of the inputs alone.
#include "slots.h"

namespace {

using namespace uf;
using slots::LEADERS;                                  // slots per wave that project() reduces with shuffles, as flush_by_slot
using slots::PX_WAVES;
constexpr int ACC_ITEMS = 8;                           // pixels per lane of both passes
constexpr int HEAD = 11;                               // int64 fields before the projections
constexpr int MAX_DIRS = 32;
constexpr int MAX_SIDE = 16384;                        // sum_xx <= 2^56, |p| < 2^30
constexpr int MAX_COMPONENT = 1 << 14;                 // |c_k|, |s_k|
constexpr int DEV = __HIP_MEMORY_SCOPE_AGENT;

struct ShapeParams {
  const int* region; const int* sizes;
  int min_pixels, image_base, h, w, D;
  long long per;                                       // h * w
  long long* rec; long long capacity;
  unsigned long long* rec_count;
  int* slot;                                           // [n][h][w] workspace
  int c[MAX_DIRS], s[MAX_DIRS];                        // by value: uniform loads from the kernel arguments
};

// what one member pixel adds to its region: the quads it is the first member of, and whether it can be extreme
struct Pixel {
  unsigned q[5];                                       // q1, q2, qd, q3, q4
  bool boundary;
};

// img: the image's region map; rg = img[y * w + x] > 0
__device__ __forceinline__ Pixel look_around(const int* img, int rg, int x, int y, int h, int w) {
  const bool up = y > 0, down = y + 1 < h, left = x > 0, right = x + 1 < w;
  const int* at = img + (long long)y * w + x;
  const bool nw = up && left && at[-w - 1] == rg, no = up && at[-w] == rg, ne = up && right && at[-w + 1] == rg;
  const bool we = left && at[-1] == rg, ea = right && at[1] == rg;
  const bool sw = down && left && at[w - 1] == rg, so = down && at[w] == rg, se = down && right && at[w + 1] == rg;
  Pixel p;
#pragma unroll
  for (int i = 0; i < 5; ++i) p.q[i] = 0u;
  // this pixel is the window's bottom-right: first member iff the three others are none
  if (!nw && !no && !we) p.q[0] += 1u;
  // bottom-left: the two above come first; the one to the right comes after
  if (!no && !ne) p.q[ea ? 1 : 0] += 1u;
  // top-right: the one to the left comes first; below-left is the diagonal, below the edge neighbour
  if (!we) p.q[sw ? (so ? 3 : 2) : (so ? 1 : 0)] += 1u;
  // top-left: always the first
  {
    const int m = (int)ea + (int)so + (int)se;
    p.q[m == 0 ? 0 : m == 1 ? (se ? 2 : 1) : m == 2 ? 3 : 4] += 1u;
  }
  p.boundary = !(nw && no && ne && we && ea && sw && so && se);
  return p;
}

// grid (pixels of one image / (PX_THREADS * ACC_ITEMS), images); every lane runs every round (the ballots want that)
__global__ __launch_bounds__(PX_THREADS) void assign_shape_slots(const ShapeParams A) {
  __shared__ unsigned cnt[PX_WAVES * ACC_ITEMS];       // kept roots per wave and round, then their exclusive prefix
  __shared__ unsigned long long block_at;
  const int n = blockIdx.y;
  const long long base = (long long)n * A.per;
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  int size[ACC_ITEMS];                                 // > 0: the pixel is the root of a kept region (min_pixels >= 1)
  unsigned long long roots[ACC_ITEMS];
#pragma unroll
  for (int k = 0; k < ACC_ITEMS; ++k) {
    const long long g = ((long long)blockIdx.x * ACC_ITEMS + k) * PX_THREADS + threadIdx.x;
    size[k] = 0;
    if (g < A.per && A.region[base + g] == (int)g + 1) {
      const int sz = A.sizes[base + g];
      if (sz >= A.min_pixels) size[k] = sz;
    }
    roots[k] = __ballot(size[k] > 0);
    if (lane == 0) cnt[wave * ACC_ITEMS + k] = (unsigned)__popcll(roots[k]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned total = 0;
#pragma unroll
    for (int i = 0; i < PX_WAVES * ACC_ITEMS; ++i) { const unsigned c = cnt[i]; cnt[i] = total; total += c; }
    block_at = total ? atomicAdd(A.rec_count, (unsigned long long)total) : 0ull;
  }
  __syncthreads();
  const unsigned long long at = block_at;
  const int F = HEAD + 2 * A.D;
#pragma unroll
  for (int k = 0; k < ACC_ITEMS; ++k) {
    const long long g = ((long long)blockIdx.x * ACC_ITEMS + k) * PX_THREADS + threadIdx.x;
    long long slot = -1;
    if (size[k] > 0) {
      slot = (long long)(at + cnt[wave * ACC_ITEMS + k] + __popcll(roots[k] & ((1ull << lane) - 1ull)));
      if (slot >= A.capacity) slot = -1;               // counted but not kept: the caller sees count > capacity
    }
    if (g < A.per) A.slot[base + g] = (int)slot;       // capacity <= 2^31 - 1
    if (slot >= 0) {
      const int x = (int)(g % A.w), y = (int)(g / A.w);
      const Pixel p = look_around(A.region + base, (int)g + 1, x, y, A.h, A.w);
      long long* r = A.rec + slot * F;
      r[0] = A.image_base + n; r[1] = g; r[2] = size[k];
      r[3] = (long long)x * x; r[4] = (long long)y * y; r[5] = (long long)x * y;
#pragma unroll
      for (int i = 0; i < 5; ++i) r[6 + i] = p.q[i];
      for (int d = 0; d < A.D; ++d) {
        const long long v = x * A.c[d] + y * A.s[d];
        r[HEAD + d] = v; r[HEAD + A.D + d] = v;
      }
    }
  }
}

struct Acc {                                           // what pixels of one slot add up to; slot < 0: nothing
  int slot;
  unsigned q[5];                                       // a block's pixels: at most 2048 * 4
  long long xx, yy, xy;
};

__device__ __forceinline__ void fold(Acc& a, const Acc& b) {
#pragma unroll
  for (int i = 0; i < 5; ++i) a.q[i] += b.q[i];
  a.xx += b.xx; a.yy += b.yy; a.xy += b.xy;
}

__device__ __forceinline__ void commit(long long* rec, int F, const Acc& a) {
  long long* r = rec + (long long)a.slot * F;
  __hip_atomic_fetch_add(&r[3], a.xx, __ATOMIC_RELAXED, DEV);
  __hip_atomic_fetch_add(&r[4], a.yy, __ATOMIC_RELAXED, DEV);
  __hip_atomic_fetch_add(&r[5], a.xy, __ATOMIC_RELAXED, DEV);
#pragma unroll
  for (int i = 0; i < 5; ++i)
    if (a.q[i]) __hip_atomic_fetch_add(&r[6 + i], (long long)a.q[i], __ATOMIC_RELAXED, DEV);
}

// the sum over the lanes with `on` (every lane of the wave calls this); `a` of the others is ignored
__device__ __forceinline__ Acc wave_fold(Acc a, bool on) {
  if (!on) {
#pragma unroll
    for (int i = 0; i < 5; ++i) a.q[i] = 0u;
    a.xx = a.yy = a.xy = 0;
  }
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    Acc b;
#pragma unroll
    for (int i = 0; i < 5; ++i) b.q[i] = __shfl_xor(a.q[i], d);
    b.xx = __shfl_xor(a.xx, d); b.yy = __shfl_xor(a.yy, d); b.xy = __shfl_xor(a.xy, d);
    fold(a, b);
  }
  return a;
}

// r: a record's pmin cell of one direction.  Lower it to v, or raise the pmax cell D further on, only where the record
// does not say so already
__device__ __forceinline__ void commit_extent(long long* r, int D, bool is_max, int v) {
  if (is_max) {
    if (__hip_atomic_load(&r[D], __ATOMIC_RELAXED, DEV) < v) __hip_atomic_fetch_max(&r[D], (long long)v, __ATOMIC_RELAXED, DEV);
  } else {
    if (__hip_atomic_load(&r[0], __ATOMIC_RELAXED, DEV) > v) __hip_atomic_fetch_min(&r[0], (long long)v, __ATOMIC_RELAXED, DEV);
  }
}

// the extremes of direction d over the lane's boundary pixels (the bits of `px`)
__device__ __forceinline__ void own_extent(const ShapeParams& A, int d, unsigned px, const int (&xs)[ACC_ITEMS],
                                           const int (&ys)[ACC_ITEMS], int& lo, int& hi) {
  const int c = A.c[d], s = A.s[d];
  lo = 0x7fffffff; hi = (int)0x80000000;
#pragma unroll
  for (int k = 0; k < ACC_ITEMS; ++k)
    if (px >> k & 1u) { const int v = xs[k] * c + ys[k] * s; lo = min(lo, v); hi = max(hi, v); }
}

// Projections of a wave: `slot` >= 0 on the lanes that hold boundary pixels of that kept region, `px` their bits.  The
// lanes that share the leading slot are reduced with shuffles, one direction after the other, LEADERS times over; a lane
// on its own, or what remains after that, hands its pixels to the whole wave.  Either way the commit is one step with
// the lanes as directions: lane d holds the minimum of direction d, lane 32 + d its maximum.  Every lane calls this.
__device__ __forceinline__ void project(const ShapeParams& A, int F, int lane, int slot, unsigned px,
                                        const int (&xs)[ACC_ITEMS], const int (&ys)[ACC_ITEMS]) {
  unsigned long long m = __ballot(slot >= 0);
  if (!m) return;                                      // wave-uniform: most waves lie inside a region or outside all
  const int dsel = lane & (MAX_DIRS - 1);
  const bool is_max = lane >= MAX_DIRS, dlane = dsel < A.D;
  const int myc = dlane ? A.c[dsel] : 0, mys = dlane ? A.s[dsel] : 0;
  for (int it = 0; it < LEADERS && m; ++it) {          // wave-uniform
    const int first = __ffsll((long long)m) - 1;
    const int lead = __shfl(slot, first);
    const bool on = slot == lead;
    const unsigned long long same = __ballot(on);
    m &= ~same;
    if (__popcll(same) < 2) continue;                  // a lane on its own has nothing to reduce: below
    int mine = 0;
    for (int d = 0; d < A.D; ++d) {
      int lo, hi;
      own_extent(A, d, on ? px : 0u, xs, ys, lo, hi);
#pragma unroll
      for (int t = 1; t < WAVE; t <<= 1) { lo = min(lo, __shfl_xor(lo, t)); hi = max(hi, __shfl_xor(hi, t)); }
      if (dsel == d) mine = is_max ? hi : lo;
    }
    if (dlane) commit_extent(A.rec + (long long)lead * F + HEAD + dsel, A.D, is_max, mine);
    if (on) slot = -1;
  }
  unsigned long long rest = __ballot(slot >= 0);
  while (rest) {                                       // wave-uniform: one lane's pixels, every direction at once
    const int src = __ffsll((long long)rest) - 1;
    rest &= rest - 1;
    const int its = __shfl(slot, src);
    const unsigned bits = (unsigned)__shfl((int)px, src);
    int lo = 0x7fffffff, hi = (int)0x80000000;
#pragma unroll
    for (int k = 0; k < ACC_ITEMS; ++k) {
      const int bx = __shfl(xs[k], src), by = __shfl(ys[k], src);
      if (bits >> k & 1u) { const int v = bx * myc + by * mys; lo = min(lo, v); hi = max(hi, v); }
    }
    if (dlane) commit_extent(A.rec + (long long)its * F + HEAD + dsel, A.D, is_max, is_max ? hi : lo);
  }
}

// Same grid as assign_shape_slots, after it.  A lane owns ACC_ITEMS CONSECUTIVE pixels and a wave 512 of them, a quarter
// of a row of a Gear image: what a lane and a wave hold is mostly one region.  (With the lanes' pixels 256 apart, as in
// the assign pass, a row that crosses a few regions of a hundred pixels makes every lane change its region several times,
// and each change is a commit.)
__global__ __launch_bounds__(PX_THREADS) void accumulate_shapes(const ShapeParams A) {
  const long long base = (long long)blockIdx.y * A.per;
  const int* img = A.region + base;
  const int lane = threadIdx.x & (WAVE - 1);
  const int F = HEAD + 2 * A.D;
  const long long g0 = ((long long)blockIdx.x * PX_THREADS + threadIdx.x) * ACC_ITEMS;
  int x = (int)(g0 % A.w), y = (int)(g0 / A.w);        // past the image for g0 >= per: not used there
  int xs[ACC_ITEMS], ys[ACC_ITEMS];
  int edge_slot = -1;                                  // the region of the lane's first boundary pixel ...
  unsigned edge_px = 0u;                               // ... and which of its pixels are boundary pixels of it
  Acc a;
  a.slot = -1;
#pragma unroll
  for (int k = 0; k < ACC_ITEMS; ++k) {
    const long long g = g0 + k;
    int slot = -1;
    if (g < A.per) {
      const int r = img[g] - 1;                        // class pixels have a region: 0 <= root < per; maps that do not
      if (r >= 0 && r < A.per && r != g)               // belong to the regions must not read elsewhere; the root pixel
        slot = A.slot[base + r];                       // is in its record already.  -1 or below the capacity
    }
    xs[k] = x; ys[k] = y;
    if (slot >= 0) {
      const Pixel px = look_around(img, img[g], x, y, A.h, A.w);
      Acc p;
      p.slot = slot;
#pragma unroll
      for (int i = 0; i < 5; ++i) p.q[i] = px.q[i];
      p.xx = (long long)x * x; p.yy = (long long)y * y; p.xy = (long long)x * y;
      if (a.slot == p.slot) {
        fold(a, p);
      } else {
        if (a.slot >= 0) commit(A.rec, F, a);          // the lane moved on to another region
        a = p;
      }
      if (px.boundary) {
        if (edge_slot < 0) edge_slot = slot;
        if (slot == edge_slot) {
          edge_px |= 1u << k;
        } else {                                       // a second region with a boundary inside 8 pixels: on its own
          long long* r = A.rec + (long long)slot * F + HEAD;
          for (int d = 0; d < A.D; ++d) {
            const int v = x * A.c[d] + y * A.s[d];
            commit_extent(r + d, A.D, false, v);
            commit_extent(r + d, A.D, true, v);
          }
        }
      }
    }
    if (++x == A.w) { x = 0; ++y; }
  }
  project(A, F, lane, edge_slot, edge_px, xs, ys);
  slots::flush_by_slot(a, [&](const Acc& s) { commit(A.rec, F, s); });
}

inline bool supported(int64_t n, int64_t h, int64_t w, int64_t D) {
  return frames_supported(n, h, w) && h <= MAX_SIDE && w <= MAX_SIDE && D >= 2 && D <= MAX_DIRS && D % 2 == 0;
}

}  // namespace

extern "C" size_t unet_measure_class_regions_workspace(int64_t n, int64_t h, int64_t w, int32_t directions) {
  if (!supported(n, h, w, directions)) return 0;
  return up16((size_t)(n * h * w) * 4);
}

extern "C" int32_t unet_measure_class_regions(const int32_t* region, const int32_t* sizes, int64_t n, int64_t h, int64_t w,
                                              int32_t min_pixels, int32_t image_base, const int32_t* direction_table,
                                              int32_t directions, int64_t* records, int64_t capacity,
                                              int64_t* record_count, void* workspace, size_t workspace_bytes,
                                              void* stream) {
  UNET_REQUIRE(region && sizes && direction_table && record_count && workspace && (records || capacity == 0),
               UNET_ERR_BAD_ARG, "unet_measure_class_regions: null pointer");
  UNET_REQUIRE(n > 0 && h > 0 && w > 0 && min_pixels >= 1 && image_base >= 0 && capacity >= 0, UNET_ERR_BAD_ARG,
               "unet_measure_class_regions: n=%lld h=%lld w=%lld min_pixels=%d image_base=%d capacity=%lld", (long long)n,
               (long long)h, (long long)w, (int)min_pixels, (int)image_base, (long long)capacity);
  const int64_t lim = (1LL << 31) - 1;
  UNET_REQUIRE(supported(n, h, w, directions) && (int64_t)image_base + n <= lim && capacity <= lim, UNET_ERR_UNSUPPORTED,
               "unet_measure_class_regions: n=%lld h=%lld w=%lld directions=%d capacity=%lld (n < 65536, at most 2^31 - 1 "
               "pixels, sides up to 16384, an even number of 2..32 directions, image indices and capacity below 2^31)",
               (long long)n, (long long)h, (long long)w, (int)directions, (long long)capacity);
  UNET_REQUIRE(workspace_bytes >= unet_measure_class_regions_workspace(n, h, w, directions), UNET_ERR_WORKSPACE,
               "unet_measure_class_regions: workspace too small");
  ShapeParams A{region, sizes, (int)min_pixels, (int)image_base, (int)h, (int)w, (int)directions, (long long)(h * w),
                (long long*)records, (long long)capacity, (unsigned long long*)record_count, (int*)workspace, {}, {}};
  for (int d = 0; d < directions; ++d) {
    const int32_t c = direction_table[2 * d], s = direction_table[2 * d + 1];
    UNET_REQUIRE(c >= -MAX_COMPONENT && c <= MAX_COMPONENT && s >= -MAX_COMPONENT && s <= MAX_COMPONENT, UNET_ERR_BAD_ARG,
                 "unet_measure_class_regions: direction %d is (%d, %d), components lie in -16384..16384", d, (int)c, (int)s);
    A.c[d] = c; A.s[d] = s;
  }
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(UNET_K_OTHER, 0.0, st, "accumulate_shapes", (double)n * h * w * 20.0);
  const dim3 grid((unsigned)cdiv64(h * w, PX_THREADS * ACC_ITEMS), (unsigned)n);
  hipLaunchKernelGGL(assign_shape_slots, grid, dim3(PX_THREADS), 0, st, A);
  int32_t rc = unet_check_launch("assign_shape_slots");
  if (rc) return rc;
  hipLaunchKernelGGL(accumulate_shapes, grid, dim3(PX_THREADS), 0, st, A);
  return unet_check_launch("accumulate_shapes");
}
