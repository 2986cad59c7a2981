// Per-defect records of labelled class regions: where every region of unet_label_class_regions lies (bounding box,
// coordinate sums for the centroid), how large it is and how sure the model was on it (sum and maximum of the per-pixel
// confidence in 16.16 fixed point).  Nothing here compares with a ground truth: segregions.hip does that.
//
// A record is DREC int64: image, class, root index, size, x0, y0, x1, y1, sum_x, sum_y, conf_sum_q, conf_max_q.  Two
// launches over the pixels, integers only:
//   assign_defect_slots   every root pixel of a kept region (size >= min_pixels) takes a slot and writes its record as
//                         the region of that one pixel: the identity fields, its own box, coordinates and q(conf).  A
//                         region of one pixel is complete with that.  The block counts its roots first (a ballot per
//                         wave and round, the counts summed through LDS) and takes all its slots with ONE atomicAdd on
//                         the device-side count: a returning atomic per wave and round on that one word is what the
//                         launch would otherwise wait for.  Every pixel leaves its slot (or -1: no root, not kept, or
//                         past the capacity) in the 4-byte-per-pixel workspace.  The whole workspace is written, so the
//                         next launch reads nothing that this call did not write.
//   accumulate_defects    every class pixel but the root finds its region's slot at the region root and folds (x, y,
//                         q(conf)) into the record with atomicMin / atomicMax / atomicAdd on int64.  Not one atomic per
//                         pixel and field: a thread folds its ACC_ITEMS pixels in registers while the slot stays the
//                         same (its pixels lie 256 apart: inside a large region they share it); slots.h's flush_by_slot
//                         then sums across the wave and the block.  A region that fills the frame costs one commit of 8
//                         atomics per block of 2048 pixels.
// The confidence is summed as segpixel.h's conf_q(v) = (uint32) rint(clamp(v, 0, 1) * 65536) (ties to even; the product
// is a scaling by a power of two, so it is exact and the TU's contraction mode cannot matter): integer sums are exact in
// any order, a float sum would depend on the order the atomics arrive in.  Apart from the record order every output is a
// function of the inputs alone.
#include "segpixel.h"
#include "slots.h"

namespace {

using namespace uf;
using namespace segpx;                                 // class_of, conf_q (segpixel.h)
constexpr int ACC_ITEMS = 8;                           // pixels per lane of both passes
constexpr int DREC = 12;                               // int64 fields of a record
using slots::PX_WAVES;

struct DescribeParams {
  const uint8_t* cls; const int* region; const int* sizes; const float* conf;
  int C, min_pixels, image_base, w;
  long long per;                                       // h * w
  long long* rec; long long capacity;
  unsigned long long* rec_count;
  int* slot;                                           // [n][h][w] workspace
};

// grid (pixels of one image / (PX_THREADS * ACC_ITEMS), images); every lane runs every round (the ballots want that)
__global__ __launch_bounds__(PX_THREADS) void assign_defect_slots(const DescribeParams A) {
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
      const long long x = g % A.w, y = g / A.w;
      const long long q = A.conf ? (long long)conf_q(A.conf[base + g]) : 0;
      long long* r = A.rec + slot * DREC;
      r[0] = A.image_base + n; r[1] = class_of(A.cls[base + g], A.C); r[2] = g; r[3] = size[k];
      r[4] = x; r[5] = y; r[6] = x; r[7] = y;
      r[8] = x; r[9] = y; r[10] = q; r[11] = q;
    }
  }
}

struct Acc {                                           // what pixels of one slot add up to; slot < 0: nothing
  int slot, x0, y0, x1, y1;
  unsigned cs, cm;                                     // a block's pixels: at most 2048 * 65536 = 2^27
  long long sx, sy;
};

__device__ __forceinline__ void fold(Acc& a, const Acc& b) {
  a.x0 = min(a.x0, b.x0); a.y0 = min(a.y0, b.y0); a.x1 = max(a.x1, b.x1); a.y1 = max(a.y1, b.y1);
  a.cs += b.cs; a.cm = max(a.cm, b.cm); a.sx += b.sx; a.sy += b.sy;
}

__device__ __forceinline__ void commit(long long* rec, const Acc& a) {
  long long* r = rec + (long long)a.slot * DREC;
  constexpr int DEV = __HIP_MEMORY_SCOPE_AGENT;
  __hip_atomic_fetch_min(&r[4], (long long)a.x0, __ATOMIC_RELAXED, DEV);
  __hip_atomic_fetch_min(&r[5], (long long)a.y0, __ATOMIC_RELAXED, DEV);
  __hip_atomic_fetch_max(&r[6], (long long)a.x1, __ATOMIC_RELAXED, DEV);
  __hip_atomic_fetch_max(&r[7], (long long)a.y1, __ATOMIC_RELAXED, DEV);
  __hip_atomic_fetch_add(&r[8], a.sx, __ATOMIC_RELAXED, DEV);
  __hip_atomic_fetch_add(&r[9], a.sy, __ATOMIC_RELAXED, DEV);
  __hip_atomic_fetch_add(&r[10], (long long)a.cs, __ATOMIC_RELAXED, DEV);
  __hip_atomic_fetch_max(&r[11], (long long)a.cm, __ATOMIC_RELAXED, DEV);
}

// the sum over the lanes with `on` (every lane of the wave calls this); `a` of the others is ignored
__device__ __forceinline__ Acc wave_fold(Acc a, bool on) {
  if (!on) { a.x0 = a.y0 = 0x7fffffff; a.x1 = a.y1 = -1; a.cs = a.cm = 0u; a.sx = a.sy = 0; }
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    Acc b;
    b.x0 = __shfl_xor(a.x0, d); b.y0 = __shfl_xor(a.y0, d); b.x1 = __shfl_xor(a.x1, d); b.y1 = __shfl_xor(a.y1, d);
    b.cs = __shfl_xor(a.cs, d); b.cm = __shfl_xor(a.cm, d); b.sx = __shfl_xor(a.sx, d); b.sy = __shfl_xor(a.sy, d);
    fold(a, b);
  }
  return a;
}

// same grid as assign_defect_slots, after it
__global__ __launch_bounds__(PX_THREADS) void accumulate_defects(const DescribeParams A) {
  const long long base = (long long)blockIdx.y * A.per;
  int slot[ACC_ITEMS];
  unsigned q[ACC_ITEMS];
#pragma unroll
  for (int k = 0; k < ACC_ITEMS; ++k) {                // the loads first: no atomic stands between them
    const long long g = ((long long)blockIdx.x * ACC_ITEMS + k) * PX_THREADS + threadIdx.x;
    slot[k] = -1;
    q[k] = 0u;
    if (g >= A.per) continue;
    const int r = A.region[base + g] - 1;              // class pixels have a region: 0 <= root < per; maps that do
    if (r < 0 || r >= A.per || r == g) continue;       // not belong to the regions must not read elsewhere; the root
                                                       // pixel is in its record already
    slot[k] = A.slot[base + r];                        // -1 or below the capacity: assign_defect_slots wrote all of it
    if (slot[k] >= 0 && A.conf) q[k] = conf_q(A.conf[base + g]);
  }
  Acc a;
  a.slot = -1;
#pragma unroll
  for (int k = 0; k < ACC_ITEMS; ++k) {
    if (slot[k] >= 0) {
      const long long g = ((long long)blockIdx.x * ACC_ITEMS + k) * PX_THREADS + threadIdx.x;
      Acc p;
      p.slot = slot[k];
      p.x0 = p.x1 = (int)(g % A.w); p.y0 = p.y1 = (int)(g / A.w);
      p.sx = p.x0; p.sy = p.y0; p.cs = p.cm = q[k];
      if (a.slot == p.slot) {
        fold(a, p);
      } else {
        if (a.slot >= 0) commit(A.rec, a);             // the thread moved on to another region
        a = p;
      }
    }
  }
  slots::flush_by_slot(a, [&](const Acc& s) { commit(A.rec, s); });
}

inline bool supported(int64_t n, int64_t h, int64_t w, int64_t C) {
  return frames_supported(n, h, w) && C >= 2 && C <= 255;
}

}  // namespace

extern "C" size_t unet_describe_class_regions_workspace(int64_t n, int64_t h, int64_t w, int32_t num_classes) {
  if (!supported(n, h, w, num_classes)) return 0;
  return up16((size_t)(n * h * w) * 4);
}

extern "C" int32_t unet_describe_class_regions(const uint8_t* classes, const int32_t* region, const int32_t* sizes,
                                               const float* conf, int64_t n, int64_t h, int64_t w, int32_t num_classes,
                                               int32_t min_pixels, int32_t image_base, int64_t* records, int64_t capacity,
                                               int64_t* record_count, void* workspace, size_t workspace_bytes,
                                               void* stream) {
  UNET_REQUIRE(classes && region && sizes && record_count && workspace && (records || capacity == 0), UNET_ERR_BAD_ARG,
               "unet_describe_class_regions: null pointer");
  UNET_REQUIRE(n > 0 && h > 0 && w > 0 && min_pixels >= 1 && image_base >= 0 && capacity >= 0, UNET_ERR_BAD_ARG,
               "unet_describe_class_regions: n=%lld h=%lld w=%lld min_pixels=%d image_base=%d capacity=%lld", (long long)n,
               (long long)h, (long long)w, (int)min_pixels, (int)image_base, (long long)capacity);
  const int64_t lim = (1LL << 31) - 1;
  UNET_REQUIRE(supported(n, h, w, num_classes) && (int64_t)image_base + n <= lim && capacity <= lim, UNET_ERR_UNSUPPORTED,
               "unet_describe_class_regions: n=%lld h=%lld w=%lld classes=%d capacity=%lld (n < 65536, at most 2^31 - 1 "
               "pixels, 2..255 classes, image indices and capacity below 2^31)", (long long)n, (long long)h, (long long)w,
               (int)num_classes, (long long)capacity);
  UNET_REQUIRE(workspace_bytes >= unet_describe_class_regions_workspace(n, h, w, num_classes), UNET_ERR_WORKSPACE,
               "unet_describe_class_regions: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  DescribeParams A{classes, region, sizes, conf, (int)num_classes, (int)min_pixels, (int)image_base, (int)w,
                   (long long)(h * w), (long long*)records, (long long)capacity, (unsigned long long*)record_count,
                   (int*)workspace};
  ProfScope prof(UNET_K_OTHER, 0.0, s, "assign_defect_slots", (double)n * h * w * (conf ? 24.0 : 20.0));
  const dim3 grid((unsigned)cdiv64(h * w, PX_THREADS * ACC_ITEMS), (unsigned)n);
  hipLaunchKernelGGL(assign_defect_slots, grid, dim3(PX_THREADS), 0, s, A);
  int32_t rc = unet_check_launch("assign_defect_slots");
  if (rc) return rc;
  hipLaunchKernelGGL(accumulate_defects, grid, dim3(PX_THREADS), 0, s, A);
  return unet_check_launch("accumulate_defects");
}
