// Overlaps of region pairs: the sparse contingency table between two region labellings.  truth_region / pred_region are
// two `region` maps of unet_label_class_regions (int32 [n][h][w], 1 + root index, 0 on background).  A pixel carries a
// pair iff both its ids are positive; every pair (truth id, pred id) of one image that some pixel carries yields one
// record (image, truth root, pred root, overlap), overlap = the pixels that carry it, whatever the regions' classes.
// segregions.hip's count_class_hits gives every region ONE number; with the pairs, which predicted regions cover a
// truth region (and so what is left of its cover above a confidence) is host arithmetic on a few records.
//
// Every lane owns PAIR_ITEMS consecutive pixels of the image's row-major order (16-byte loads where the maps allow it).
// Launches, integers only, no workgroup waits on another:
//   count_pair_starts   (unet_region_pair_bound) a pixel that carries a pair and has x == 0 or another pair (or none)
//                       to its left is a start.  The row-major first pixel of every distinct pair is a start, so the
//                       starts of an image bound its distinct pairs from above; there are about as many as the overlaps
//                       have rows.  The block sums its lanes (shuffles, then LDS) and adds once to the image's count: a wave
//                       each on that one word is what the launch would otherwise wait for.
//   fill_pair_table     (unet_region_pairs, after a memset of the tables) one open-addressing table per image:
//                       `capacity` (a power of two) 64-bit keys truth id << 32 | pred id (never 0: 0 is an empty slot) and as many
//                       int32 counts.  A lane merges its pixels into runs of one key; when a run ends, the lanes of the
//                       wave that end a run of the first such lane's key sum their lengths with shuffles and that lane
//                       inserts once; so do the lanes of the next pending key, LEADERS times over, and what is left
//                       after that inserts its own.  The FIRST sums of a lane's LAST run (inside an overlap:
//                       its only one) go through LDS first, where one thread folds the waves that share a key: a large
//                       overlap costs one insert per block of 2048 pixels.  Insert: from the key's hash,
//                       atomicCAS(0 -> key) on the slot's key; the slot that holds the key (mine or somebody's before
//                       me) gets an integer atomicAdd of the length; another key: next slot.  No slot in `capacity`
//                       steps: the run's pixels are added to *overflow and dropped.
//   emit_pair_records   a thread per slot: every used slot appends (image_base + image, truth id - 1, pred id - 1,
//                       count) to `records`; the index comes from one atomicAdd per wave on *count, so the order is arbitrary
//                       and the caller sorts.  A record at record_cap or beyond is counted and not written.
// Termination: every loop is counted.  The probe loop runs at most `capacity` steps whatever other threads do: a slot's
// key is written once (0 -> key) and never changes again, a lane that loses the CAS reads the winner's key from the
// atomic's return value and either shares the slot or moves on; nobody waits for anybody.  The ids are only compared
// and packed, never used as an index: maps that are not region maps cannot send an access anywhere.  Integer adds are exact
// in any order, so the SET of records is a function of the two maps alone (which slot a key lands in is not, and does
// not show).
#include "unionfind.h"

namespace {

using namespace uf;
constexpr int PAIR_ITEMS = 8;                          // consecutive pixels per lane
constexpr int PAIR_BLOCK = PX_THREADS * PAIR_ITEMS;    // pixels per block
constexpr int PREC = 4;                                // int32 fields of a record
constexpr int PX_WAVES = PX_THREADS / WAVE;
constexpr int LEADERS = 4;                             // keys per wave and round that are summed with shuffles
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef unsigned long long u64;

// v[k] = map[g0 + k], 0 at and beyond per.  VEC: the image's plane starts on 16 bytes and per % 4 == 0, so a group of
// four pixels lies inside the plane or outside it as a whole (g0 % 4 == 0).
template <bool VEC>
__device__ __forceinline__ void load_items(const int* __restrict__ map, long long g0, long long per,
                                           int (&v)[PAIR_ITEMS]) {
  if constexpr (VEC) {
#pragma unroll
    for (int j = 0; j < PAIR_ITEMS; j += 4) {
      i32x4 q = {0, 0, 0, 0};
      if (g0 + j < per) q = *reinterpret_cast<const i32x4*>(map + g0 + j);
      v[j] = q[0]; v[j + 1] = q[1]; v[j + 2] = q[2]; v[j + 3] = q[3];
    }
  } else {
#pragma unroll
    for (int k = 0; k < PAIR_ITEMS; ++k) v[k] = g0 + k < per ? map[g0 + k] : 0;
  }
}

__device__ __forceinline__ u64 pair_key(int t, int p) {
  return (t > 0 && p > 0) ? ((u64)(unsigned)t << 32) | (u64)(unsigned)p : 0ull;
}

struct BoundParams {
  const int* treg; const int* preg;
  int w; long long per;
  u64* bound;                                          // [n]
};

// grid (pixels of one image / PAIR_BLOCK, images)
template <bool VEC>
__global__ __launch_bounds__(PX_THREADS) void count_pair_starts(const BoundParams A) {
  __shared__ int part[PX_WAVES];
  const int n = blockIdx.y;
  const long long base = (long long)n * A.per;
  const long long g0 = ((long long)blockIdx.x * PX_THREADS + threadIdx.x) * PAIR_ITEMS;
  int starts = 0;
  if (g0 < A.per) {                                    // g0 < 2^31
    int t[PAIR_ITEMS], p[PAIR_ITEMS];
    load_items<VEC>(A.treg + base, g0, A.per, t);
    load_items<VEC>(A.preg + base, g0, A.per, p);
    int x = (int)((unsigned)g0 % (unsigned)A.w);
    u64 left = x > 0 ? pair_key(A.treg[base + g0 - 1], A.preg[base + g0 - 1]) : 0ull;      // x > 0: g0 - 1 >= 0
#pragma unroll
    for (int k = 0; k < PAIR_ITEMS; ++k) {
      const u64 key = pair_key(t[k], p[k]);            // 0 beyond the plane
      if (key && (x == 0 || key != left)) ++starts;
      left = key;
      if (++x == A.w) x = 0;
    }
  }
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) starts += __shfl_xor(starts, d);
  if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = starts;
  __syncthreads();
  if (threadIdx.x != 0) return;
  starts = 0;
#pragma unroll
  for (int i = 0; i < PX_WAVES; ++i) starts += part[i];
  if (starts) atomicAdd(&A.bound[n], (u64)starts);
}

struct PairParams {
  const int* treg; const int* preg;
  long long per;
  long long capacity;                                  // slots per image, a power of two
  u64* keys;                                           // [n][capacity]
  int* counts;                                         // [n][capacity]
  u64* overflow;
  int image_base;
  int* rec; long long record_cap;
  u64* rec_count;
};

__device__ __forceinline__ long long slot_of(u64 key, long long mask) {
  key *= 0x9E3779B97F4A7C15ull;                        // Fibonacci hashing: the high bits mix both ids
  return (long long)((key >> 24) & (u64)mask);         // capacity <= 2^30
}

// one lane, `pixels` pixels of `key` (not 0): at most `capacity` probes, see the header
__device__ __forceinline__ void insert_pair(u64* keys, int* counts, long long capacity, u64 key, int pixels,
                                            u64* overflow) {
  const long long mask = capacity - 1;
  long long s = slot_of(key, mask);
  for (long long step = 0; step < capacity; ++step) {
    u64 cur = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0ull) {
      cur = atomicCAS(&keys[s], 0ull, key);            // what was there: 0 (the slot is mine now) or the winner's key
      if (cur == 0ull) cur = key;
    }
    if (cur == key) {
      atomicAdd(&counts[s], pixels);
      return;
    }
    s = (s + 1) & mask;
  }
  atomicAdd(overflow, (u64)pixels);
}

// Every lane of the wave calls this; `on`: the lane ends a run of `pixels` pixels of `key`.  LEADERS times over, the lanes
// that share the key of the first pending lane sum their lengths with shuffles and that lane inserts the sum; what is
// left after that (a wave across more than LEADERS overlaps) inserts its own.  A wave across the border of two large
// overlaps would otherwise send every lane of the second one to the same slot.  DEPOSIT: the first sum is not inserted
// but left in (dep_key, dep_sum), the same in every lane, for the block to fold.
template <bool DEPOSIT>
__device__ __forceinline__ void wave_insert(u64* keys, int* counts, long long capacity, u64 key, int pixels, bool on,
                                            int lane, u64* overflow, u64& dep_key, int& dep_sum) {
  u64 m = __ballot(on);
  for (int it = 0; it < LEADERS && m; ++it) {          // wave-uniform
    const int first = __ffsll((long long)m) - 1;
    const u64 lead = __shfl(key, first);
    const bool same = on && key == lead;
    const u64 sm = __ballot(same);
    int sum = same ? pixels : 0;
    if (sm != (1ull << first)) {                       // wave-uniform: somebody shares the leader's key
#pragma unroll
      for (int d = 1; d < WAVE; d <<= 1) sum += __shfl_xor(sum, d);
    }
    if (DEPOSIT && it == 0) {
      dep_key = lead;
      dep_sum = __shfl(sum, first);
    } else if (lane == first) {
      insert_pair(keys, counts, capacity, lead, sum, overflow);
    }
    if (same) on = false;
    m &= ~sm;
  }
  if (on) insert_pair(keys, counts, capacity, key, pixels, overflow);
}

// grid (pixels of one image / PAIR_BLOCK, images); every lane runs every round (the ballots want that)
template <bool VEC>
__global__ __launch_bounds__(PX_THREADS) void fill_pair_table(const PairParams A) {
  __shared__ u64 part_key[PX_WAVES];                   // the shared sum of every wave's last round; key 0: none
  __shared__ int part_sum[PX_WAVES];
  const int n = blockIdx.y;
  const long long base = (long long)n * A.per;
  const long long g0 = ((long long)blockIdx.x * PX_THREADS + threadIdx.x) * PAIR_ITEMS;
  const int lane = threadIdx.x & (WAVE - 1);
  u64* keys = A.keys + (long long)n * A.capacity;
  int* counts = A.counts + (long long)n * A.capacity;
  int t[PAIR_ITEMS], p[PAIR_ITEMS];
  load_items<VEC>(A.treg + base, g0, A.per, t);        // all 0 for a lane beyond the plane
  load_items<VEC>(A.preg + base, g0, A.per, p);
  u64 key[PAIR_ITEMS];
#pragma unroll
  for (int k = 0; k < PAIR_ITEMS; ++k) key[k] = pair_key(t[k], p[k]);
  int run = 0, dep_sum = 0;
  u64 dep_key = 0ull;
#pragma unroll
  for (int k = 0; k < PAIR_ITEMS - 1; ++k) {
    ++run;
    const bool ends = key[k + 1] != key[k];
    wave_insert<false>(keys, counts, A.capacity, key[k], run, ends && key[k] != 0ull, lane, A.overflow, dep_key,
                       dep_sum);
    if (ends) run = 0;
  }
  ++run;
  wave_insert<true>(keys, counts, A.capacity, key[PAIR_ITEMS - 1], run, key[PAIR_ITEMS - 1] != 0ull, lane, A.overflow,
                    dep_key, dep_sum);
  // the block: the waves' last sums, folded where they share a key
  if (lane == 0) { part_key[threadIdx.x / WAVE] = dep_key; part_sum[threadIdx.x / WAVE] = dep_sum; }
  __syncthreads();
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int i = 0; i < PX_WAVES; ++i) {
    const u64 k = part_key[i];
    if (k == 0ull) continue;
    int sum = part_sum[i];
#pragma unroll
    for (int j = i + 1; j < PX_WAVES; ++j)
      if (part_key[j] == k) { sum += part_sum[j]; part_key[j] = 0ull; }
    insert_pair(keys, counts, A.capacity, k, sum, A.overflow);
  }
}

// grid (capacity / PX_THREADS, images), after fill_pair_table
__global__ __launch_bounds__(PX_THREADS) void emit_pair_records(const PairParams A) {
  const int n = blockIdx.y;
  const long long s = (long long)blockIdx.x * PX_THREADS + threadIdx.x;
  const int lane = threadIdx.x & (WAVE - 1);
  const u64 key = s < A.capacity ? A.keys[(long long)n * A.capacity + s] : 0ull;
  const bool used = key != 0ull;
  const u64 m = __ballot(used);
  if (!m) return;                                      // wave-uniform
  const int first = __ffsll((long long)m) - 1;
  u64 at = 0;
  if (lane == first) at = atomicAdd(A.rec_count, (u64)__popcll(m));
  at = __shfl(at, first);
  if (!used) return;
  const u64 slot = at + (u64)__popcll(m & ((1ull << lane) - 1ull));
  if (slot >= (u64)A.record_cap) return;               // counted but not kept: the caller sees count > record_cap
  int* r = A.rec + (long long)slot * PREC;
  r[0] = A.image_base + n; r[1] = (int)(key >> 32) - 1; r[2] = (int)(key & 0xffffffffull) - 1;
  r[3] = A.counts[(long long)n * A.capacity + s];
}

constexpr int64_t MAX_CAPACITY = 1LL << 30;
inline bool capacity_ok(int64_t capacity) { return capacity >= 1 && (capacity & (capacity - 1)) == 0; }
inline bool table_supported(int64_t n, int64_t capacity) {
  return n > 0 && n < 65536 && capacity <= MAX_CAPACITY && n <= (1LL << 40) / capacity;
}
// 16-byte loads: both planes of every image start on 16 bytes
inline bool vec_ok(const void* a, const void* b, int64_t per) {
  return (((uintptr_t)a | (uintptr_t)b) & 15) == 0 && per % 4 == 0;
}

}  // namespace

extern "C" int32_t unet_region_pair_bound(const int32_t* truth_region, const int32_t* pred_region, int64_t n, int64_t h,
                                          int64_t w, int64_t* bound, void* stream) {
  UNET_REQUIRE(truth_region && pred_region && bound, UNET_ERR_BAD_ARG, "unet_region_pair_bound: null pointer");
  UNET_REQUIRE(n > 0 && h > 0 && w > 0, UNET_ERR_BAD_ARG, "unet_region_pair_bound: n=%lld h=%lld w=%lld", (long long)n,
               (long long)h, (long long)w);
  UNET_REQUIRE(frames_supported(n, h, w), UNET_ERR_UNSUPPORTED,
               "unet_region_pair_bound: n=%lld h=%lld w=%lld (n < 65536, at most 2^31 - 1 pixels)", (long long)n,
               (long long)h, (long long)w);
  hipStream_t s = (hipStream_t)stream;
  BoundParams A{truth_region, pred_region, (int)w, (long long)(h * w), (u64*)bound};
  ProfScope prof(UNET_K_OTHER, 0.0, s, "count_pair_starts", (double)n * h * w * 8.0);
  const dim3 grid((unsigned)cdiv64(h * w, PAIR_BLOCK), (unsigned)n);
  if (vec_ok(truth_region, pred_region, h * w))
    hipLaunchKernelGGL(count_pair_starts<true>, grid, dim3(PX_THREADS), 0, s, A);
  else
    hipLaunchKernelGGL(count_pair_starts<false>, grid, dim3(PX_THREADS), 0, s, A);
  return unet_check_launch("count_pair_starts");
}

extern "C" size_t unet_region_pairs_workspace(int64_t n, int64_t capacity) {
  if (!capacity_ok(capacity) || !table_supported(n, capacity)) return 0;
  return up16((size_t)(n * capacity) * 12);
}

extern "C" int32_t unet_region_pairs(const int32_t* truth_region, const int32_t* pred_region, int64_t n, int64_t h,
                                     int64_t w, int64_t capacity, int32_t image_base, int32_t* records,
                                     int64_t record_cap, int64_t* count, int64_t* overflow, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  UNET_REQUIRE(truth_region && pred_region && count && overflow && workspace && (records || record_cap == 0),
               UNET_ERR_BAD_ARG, "unet_region_pairs: null pointer");
  UNET_REQUIRE(n > 0 && h > 0 && w > 0 && image_base >= 0 && record_cap >= 0, UNET_ERR_BAD_ARG,
               "unet_region_pairs: n=%lld h=%lld w=%lld image_base=%d record_cap=%lld", (long long)n, (long long)h,
               (long long)w, (int)image_base, (long long)record_cap);
  UNET_REQUIRE(capacity_ok(capacity), UNET_ERR_BAD_ARG, "unet_region_pairs: capacity=%lld is not a power of two",
               (long long)capacity);
  const int64_t lim = (1LL << 31) - 1;
  UNET_REQUIRE(frames_supported(n, h, w) && table_supported(n, capacity) && (int64_t)image_base + n <= lim &&
                   record_cap <= lim,
               UNET_ERR_UNSUPPORTED,
               "unet_region_pairs: n=%lld h=%lld w=%lld capacity=%lld record_cap=%lld (n < 65536, at most 2^31 - 1 pixels, capa"
               "city <= 2^30, n * capacity <= 2^40, image indices and record_cap below 2^31)", (long long)n,
               (long long)h, (long long)w, (long long)capacity, (long long)record_cap);
  const size_t need = unet_region_pairs_workspace(n, capacity);
  UNET_REQUIRE(workspace_bytes >= need, UNET_ERR_WORKSPACE, "unet_region_pairs: workspace too small");
  UNET_REQUIRE(((uintptr_t)workspace & 7) == 0, UNET_ERR_BAD_ARG, "unet_region_pairs: workspace is not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const long long slots = (long long)(n * capacity);
  UNET_REQUIRE(hipMemsetAsync(workspace, 0, (size_t)slots * 12, s) == hipSuccess, UNET_ERR_LAUNCH,
               "unet_region_pairs: memset failed");
  PairParams A{truth_region, pred_region, (long long)(h * w), (long long)capacity, (u64*)workspace,
               (int*)((u64*)workspace + slots), (u64*)overflow, (int)image_base, records, (long long)record_cap,
               (u64*)count};
  // the maps once, the tables cleared, filled (about a slot per record) and read, the records
  ProfScope prof(UNET_K_OTHER, 0.0, s, "fill_pair_table", (double)n * h * w * 8.0 + (double)slots * 24.0);
  const dim3 grid((unsigned)cdiv64(h * w, PAIR_BLOCK), (unsigned)n);
  if (vec_ok(truth_region, pred_region, h * w))
    hipLaunchKernelGGL(fill_pair_table<true>, grid, dim3(PX_THREADS), 0, s, A);
  else
    hipLaunchKernelGGL(fill_pair_table<false>, grid, dim3(PX_THREADS), 0, s, A);
  int32_t rc = unet_check_launch("fill_pair_table");
  if (rc) return rc;
  hipLaunchKernelGGL(emit_pair_records, dim3((unsigned)cdiv64(capacity, PX_THREADS), (unsigned)n), dim3(PX_THREADS), 0, s,
                     A);
  return unet_check_launch("emit_pair_records");
}
