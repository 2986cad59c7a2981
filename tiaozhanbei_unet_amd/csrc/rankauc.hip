// Pixel-level AUROC / AUPRC of the anomaly branch's evaluation (reference src/test.py:172-178 evaluate_results ->
// src/utils.py:97-108 calculate_pixel_metrics -> :84-91 roc_auc_score and auc(precision_recall_curve)).  The reference
// copies every anomaly map to the host and sorts all pixels twice in sklearn; here the pixels never leave the device:
//   rank_auc_append    two walks over pred / truth (selected images only): every finite score becomes an order-preserving
//                      uint32 key, compacted into the positive (truth > 0.5) or the negative key array; a counting walk,
//                      one integer atomicAdd per block and class, then a writing walk ranked by ballot; non-finite
//                      scores are counted.
//   radix_hist, radix_scan, radix_scatter
//                      keys-only LSD radix sort of both arrays in the same launches (blockIdx spans the two): 8-bit
//                      digits, 4 passes of a per-block 256-bin histogram (digit-major table; digit totals by integer
//                      atomics), an exclusive scan of that table (a block per digit) and a stable scatter (block-local
//                      ranks in input order from wave ballots).  Separate launches: no workgroup waits on another.
//   auc_curve          one lane per element of the sorted positive array; at the head of each run of equal keys, a
//                      gallop in the positive array and binary searches in the negative one give pos_v, #neg<v, neg_v
//                      and the counts above v: the Mann-Whitney numerator (uint64, exact) and the AUPRC trapezoids (fp64).
//   auc_finalize       one block: ordered sums of the per-block partials; AUROC = numerator / (2 P N) correctly rounded.
// No float atomics: the sorted arrays are a function of the pixel multiset and every partition below a function of
// (P, N), so results are bitwise identical whatever the batch split, image order or run.
#include "common.h"

namespace {

constexpr int AP_THREADS = 256;
constexpr int AP_WAVES = AP_THREADS / WAVE;
constexpr int RS_THREADS = 256;
constexpr int RS_WAVES = RS_THREADS / WAVE;
constexpr int RS_ITEMS = 8;                            // keys per lane per scatter tile
constexpr int RS_TILE = RS_THREADS * RS_ITEMS;
constexpr int RS_GRID = 768;                           // both arrays together: 3 blocks per CU (LDS) on 256 CUs
constexpr int SCAN_THREADS = 1024;                     // >= the blocks of one array (RS_GRID + 1)
constexpr int CV_THREADS = 256;
constexpr int CV_MAX_BLOCKS = 4096;
constexpr int FIN_THREADS = 256;

// ---- append ------------------------------------------------------------------------------------------------------------
struct AppendParams {
  const float* pred; const float* truth; const uint8_t* select;
  long long per; int bpi;
  uint32_t* keys; long long cap;                       // positives grow from keys[0], negatives from keys[cap - 1] down
  unsigned long long* counts;                          // {positives, negatives, non-finite}
};

// order-preserving key of a finite float: -0.0 == +0.0 first, then sign-magnitude -> unsigned order
__device__ __forceinline__ uint32_t score_key(float x) {
  uint32_t u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <int V>
__device__ __forceinline__ void load_units(const float* p, const float* t, long long u, float (&x)[V], float (&y)[V]) {
  if constexpr (V == 4) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p + 4 * u);
    const f32x4 c = *reinterpret_cast<const f32x4*>(t + 4 * u);
#pragma unroll
    for (int j = 0; j < 4; ++j) { x[j] = a[j]; y[j] = c[j]; }
  } else {
    x[0] = p[u]; y[0] = t[u];
  }
}
__device__ __forceinline__ bool finite_score(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// A block owns a fixed unit range of one image and walks it twice: the first walk counts its positives, negatives and
// non-finite scores (one atomicAdd per class for the whole block reserves its output ranges: a per-wave atomic on
// one address serialised the whole pass), the second walks the same units in the same lane order and writes the
// keys, ranked by ballot within each wave from the wave's base.  The second read mostly hits the caches.
template <int V>
__global__ __launch_bounds__(AP_THREADS) void rank_auc_append(const AppendParams A) {
  __shared__ unsigned int wcnt[3][AP_WAVES];
  __shared__ unsigned long long wbase[2][AP_WAVES];
  const int n = blockIdx.y, b = blockIdx.x;
  if (A.select && !A.select[n]) return;                // block-uniform
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const unsigned long long lower = (1ull << lane) - 1ull;
  const long long units = A.per / V;                   // V divides per
  const long long per_b = cdiv64(units, A.bpi);
  const long long u0 = b * per_b, u1 = min(u0 + per_b, units);
  const float* p = A.pred + (long long)n * A.per;
  const float* t = A.truth + (long long)n * A.per;

  unsigned int cp = 0, cn = 0, cf = 0;
  for (long long u = u0 + threadIdx.x; u < u1; u += AP_THREADS) {
    float x[V], y[V];
    load_units<V>(p, t, u, x, y);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const bool fin = finite_score(x[j]), pos = y[j] > 0.5f;
      cp += fin && pos;
      cn += fin && !pos;
      cf += !fin;
    }
  }
#pragma unroll
  for (int m = WAVE / 2; m >= 1; m >>= 1) {
    cp += __shfl_xor(cp, m);
    cn += __shfl_xor(cn, m);
    cf += __shfl_xor(cf, m);
  }
  if (lane == 0) { wcnt[0][wave] = cp; wcnt[1][wave] = cn; wcnt[2][wave] = cf; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long tp = 0, tn = 0, tf = 0;
#pragma unroll
    for (int w = 0; w < AP_WAVES; ++w) { tp += wcnt[0][w]; tn += wcnt[1][w]; tf += wcnt[2][w]; }
    unsigned long long bp = tp ? atomicAdd(&A.counts[0], tp) : 0ull;
    unsigned long long bn = tn ? atomicAdd(&A.counts[1], tn) : 0ull;
    if (tf) atomicAdd(&A.counts[2], tf);
#pragma unroll
    for (int w = 0; w < AP_WAVES; ++w) {
      wbase[0][w] = bp; bp += wcnt[0][w];
      wbase[1][w] = bn; bn += wcnt[1][w];
    }
  }
  __syncthreads();
  if (wcnt[0][wave] + wcnt[1][wave] == 0) return;     // wave-uniform: nothing of this wave's to write
  unsigned long long pbase = wbase[0][wave], nbase = wbase[1][wave];
  // every lane of the wave runs the same trip count (the ballots need the whole wave)
  for (long long base = u0; base < u1; base += AP_THREADS) {
    const long long u = base + threadIdx.x;
    const bool in = u < u1;
    float x[V], y[V];
    if (in) load_units<V>(p, t, u, x, y);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const bool fin = in && finite_score(x[j]), pos = in && y[j] > 0.5f;
      const unsigned long long bp = __ballot(fin && pos), bn = __ballot(fin && !pos);
      if (fin && pos) {
        const unsigned long long i = pbase + __popcll(bp & lower);
        if (i < (unsigned long long)A.cap) A.keys[i] = score_key(x[j]);
      } else if (fin) {
        const unsigned long long i = nbase + __popcll(bn & lower);
        if (i < (unsigned long long)A.cap) A.keys[A.cap - 1 - (long long)i] = score_key(x[j]);
      }
      pbase += __popcll(bp);
      nbase += __popcll(bn);
    }
  }
}

inline int append_bpi(long long n, long long units) {
  long long b = cdiv64(units, 4 * AP_THREADS);          // >= 4 units per lane
  const long long cap = 2048 / n > 0 ? 2048 / n : 1;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

// ---- radix sort ----------------------------------------------------------------------------------------------------------
struct SortSeg {
  const uint32_t* src; uint32_t* dst;
  long long n, per;                                    // per: keys per block, a multiple of RS_TILE
  int blocks;
  uint32_t* table;                                     // [256][blocks]: digit counts, then exclusive offsets
  uint32_t* tot;                                       // [256] keys per digit in this pass (zeroed by the caller)
};
struct SortParams { SortSeg s[2]; int shift; };

__device__ __forceinline__ int seg_of(const SortParams& P, int& lb) {
  lb = blockIdx.x;
  if (lb < P.s[0].blocks) return 0;
  lb -= P.s[0].blocks;
  return 1;
}

__global__ __launch_bounds__(RS_THREADS) void radix_hist(const SortParams P) {
  __shared__ uint32_t h[RS_WAVES][256];
  int lb;
  const SortSeg S = P.s[seg_of(P, lb)];
  const int wave = threadIdx.x / WAVE;
  for (int i = threadIdx.x; i < RS_WAVES * 256; i += RS_THREADS) (&h[0][0])[i] = 0;
  __syncthreads();
  const long long start = lb * S.per, end = min(start + S.per, S.n);
  for (long long i = start + 4 * threadIdx.x; i < end; i += 4 * RS_THREADS) {   // start is 16-byte aligned
    if (i + 4 <= end) {
      const u32x4 k = *reinterpret_cast<const u32x4*>(S.src + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) atomicAdd(&h[wave][(k[j] >> P.shift) & 255u], 1u);
    } else {
      for (long long q = i; q < end; ++q) atomicAdd(&h[wave][(S.src[q] >> P.shift) & 255u], 1u);
    }
  }
  __syncthreads();
  const int d = threadIdx.x;
  uint32_t c = 0;
#pragma unroll
  for (int w = 0; w < RS_WAVES; ++w) c += h[w][d];
  S.table[(size_t)d * S.blocks + lb] = c;
  if (c) atomicAdd(&S.tot[d], c);                      // integer: exact in any order
}

// grid (256 digits, 2 arrays), a thread per block of the sorting grid: offset of (digit d, block b) = the keys of every
// smaller digit (the pass's digit totals) + the digit-d keys of blocks < b (a block-wide scan of the row)
__global__ __launch_bounds__(SCAN_THREADS) void radix_scan(const SortParams P) {
  __shared__ uint32_t red[SCAN_THREADS / WAVE], wsum[SCAN_THREADS / WAVE];
  const SortSeg S = P.s[blockIdx.y];
  if (S.blocks == 0) return;                           // block-uniform
  const int d = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  uint32_t below = tid < d ? S.tot[tid] : 0u;
#pragma unroll
  for (int m = WAVE / 2; m >= 1; m >>= 1) below += __shfl_xor(below, m);
  uint32_t* row = S.table + (size_t)d * S.blocks;
  const uint32_t c = tid < S.blocks ? row[tid] : 0u;
  uint32_t x = c;                                      // inclusive scan within the wave
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const uint32_t y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  if (lane == 0) red[wave] = below;
  if (lane == WAVE - 1) wsum[wave] = x;
  __syncthreads();
  uint32_t base = 0;
#pragma unroll
  for (int w = 0; w < SCAN_THREADS / WAVE; ++w) base += red[w] + (w < wave ? wsum[w] : 0u);
  if (tid < S.blocks) row[tid] = base + x - c;
}

// Stable: a tile is RS_ITEMS sub-tiles of 256 consecutive keys; the key at t0 + j*256 + w*64 + lane is ranked after
// every earlier (j, w) and, within its wave, after the lower lanes with the same digit (8 ballots give those peers).
__global__ __launch_bounds__(RS_THREADS) void radix_scatter(const SortParams P) {
  __shared__ uint16_t cnt[RS_ITEMS][RS_WAVES][256];    // per (sub-tile, wave) digit counts; zero between tiles
  __shared__ uint32_t off[RS_ITEMS][RS_WAVES][256];    // their global start offsets
  __shared__ uint32_t run[256];                        // next free position of each digit in this block's output
  int lb;
  const SortSeg S = P.s[seg_of(P, lb)];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE, tid = threadIdx.x;
  const unsigned long long lower = (1ull << lane) - 1ull;
  for (int i = tid; i < RS_ITEMS * RS_WAVES * 256; i += RS_THREADS) (&cnt[0][0][0])[i] = 0;
  run[tid] = S.table[(size_t)tid * S.blocks + lb];
  __syncthreads();
  const long long start = lb * S.per, end = min(start + S.per, S.n);
  for (long long t0 = start; t0 < end; t0 += RS_TILE) {
    uint32_t k[RS_ITEMS];
    int dig[RS_ITEMS], rank[RS_ITEMS];
#pragma unroll
    for (int j = 0; j < RS_ITEMS; ++j) {
      const long long i = t0 + j * RS_THREADS + tid;
      k[j] = i < end ? S.src[i] : 0u;
    }
#pragma unroll
    for (int j = 0; j < RS_ITEMS; ++j) {
      const bool valid = t0 + j * RS_THREADS + tid < end;
      const int d = (int)((k[j] >> P.shift) & 255u);
      unsigned long long peers = __ballot(valid);
#pragma unroll
      for (int bit = 0; bit < 8; ++bit) {
        const unsigned long long ones = __ballot((d >> bit) & 1);
        peers &= ((d >> bit) & 1) ? ones : ~ones;
      }
      dig[j] = valid ? d : -1;
      rank[j] = __popcll(peers & lower);
      if (valid && rank[j] == 0) cnt[j][wave][d] = (uint16_t)__popcll(peers);
    }
    __syncthreads();
    {
      uint32_t r = run[tid];
#pragma unroll
      for (int j = 0; j < RS_ITEMS; ++j) {
#pragma unroll
        for (int w = 0; w < RS_WAVES; ++w) {
          off[j][w][tid] = r;
          r += cnt[j][w][tid];
          cnt[j][w][tid] = 0;
        }
      }
      run[tid] = r;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RS_ITEMS; ++j) {
      if (dig[j] >= 0) {
        const uint32_t q = off[j][wave][dig[j]] + (uint32_t)rank[j];
        if (q < (unsigned long long)S.n) S.dst[q] = k[j];
      }
    }
    // the next tile's ballots write only cnt (zeroed above); off is rewritten after its first barrier
  }
}

// ---- curve -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long lower_bound(const uint32_t* a, long long lo, long long hi, uint32_t v) {
  while (lo < hi) {
    const long long m = lo + ((hi - lo) >> 1);
    if (a[m] < v) lo = m + 1; else hi = m;
  }
  return lo;
}
__device__ __forceinline__ long long upper_bound(const uint32_t* a, long long lo, long long hi, uint32_t v) {
  while (lo < hi) {
    const long long m = lo + ((hi - lo) >> 1);
    if (a[m] <= v) lo = m + 1; else hi = m;
  }
  return lo;
}

__global__ __launch_bounds__(CV_THREADS) void auc_curve(const uint32_t* __restrict__ pos, long long P,
                                                        const uint32_t* __restrict__ neg, long long N, long long per,
                                                        unsigned long long* __restrict__ pnum, double* __restrict__ ppr) {
  __shared__ unsigned long long rn[CV_THREADS / WAVE];
  __shared__ double rp[CV_THREADS / WAVE];
  __shared__ long long nrange[2];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const long long start = blockIdx.x * per, end = min(start + per, P);
  if (threadIdx.x == 0) {                              // every value of this block lies in [pos[start], pos[end - 1]]
    nrange[0] = lower_bound(neg, 0, N, pos[start]);
    nrange[1] = upper_bound(neg, nrange[0], N, pos[end - 1]);
  }
  __syncthreads();
  const long long nlo = nrange[0], nhi = nrange[1];
  unsigned long long num = 0;
  double pr = 0.0;
  for (long long i = start + threadIdx.x; i < end; i += CV_THREADS) {
    const uint32_t v = pos[i];
    if (i > 0 && pos[i - 1] == v) continue;            // not the head of its run
    long long last = i, probe = i + 1, step = 1;       // gallop to the run's end: most runs are short
    while (probe < P && pos[probe] == v) { last = probe; probe = last + step; step <<= 1; }
    const long long e = upper_bound(pos, last + 1, min(probe, P), v);
    const long long lo = lower_bound(neg, nlo, nhi, v);
    const long long hi = upper_bound(neg, lo, nhi, v);
    const long long pv = e - i, nv = hi - lo, ap = P - e, an = N - hi;
    num += (unsigned long long)pv * (unsigned long long)(2 * lo + nv);
    const double cur = (double)(ap + pv) / (double)(ap + pv + an + nv);
    const double prev = ap + an > 0 ? (double)ap / (double)(ap + an) : 1.0;
    pr += ((double)pv / (double)P) * ((cur + prev) * 0.5);
  }
#pragma unroll
  for (int m = WAVE / 2; m >= 1; m >>= 1) {
    num += __shfl_xor(num, m);
    pr += __shfl_xor(pr, m);
  }
  if (lane == 0) { rn[wave] = num; rp[wave] = pr; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long a = 0;
    double b = 0.0;
#pragma unroll
    for (int w = 0; w < CV_THREADS / WAVE; ++w) { a += rn[w]; b += rp[w]; }
    pnum[blockIdx.x] = a;
    ppr[blockIdx.x] = b;
  }
}

// num / den rounded once to the nearest fp64 (ties to even); 0 <= num <= den < 2^62.  Long division: the remainder stays
// below 2 den < 2^63, so nothing overflows.
__device__ double ratio_rn(unsigned long long num, unsigned long long den) {
  if (num == 0) return 0.0;
  int e = 0;
  unsigned long long r = num;
  while (r < den) { r <<= 1; --e; }                    // num / den = (r / den) 2^e, r / den in [1, 2)
  unsigned long long q = 0;
  for (int i = 0; i < 54; ++i) {                       // the leading 1, 52 fraction bits and the rounding bit
    q <<= 1;
    if (r >= den) { q |= 1; r -= den; }
    r <<= 1;
  }
  unsigned long long m = q >> 1;
  if ((q & 1) && (r != 0 || (m & 1))) ++m;             // m == 2^53 after a carry is still exact
  return ldexp((double)m, e - 52);
}

__global__ __launch_bounds__(FIN_THREADS) void auc_finalize(const unsigned long long* __restrict__ pnum,
                                                            const double* __restrict__ ppr, int parts, long long P,
                                                            long long N, double* __restrict__ out) {
  __shared__ unsigned long long rn[FIN_THREADS / WAVE];
  __shared__ double rp[FIN_THREADS / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  unsigned long long num = 0;
  double pr = 0.0;
  for (int b = threadIdx.x; b < parts; b += FIN_THREADS) { num += pnum[b]; pr += ppr[b]; }
#pragma unroll
  for (int m = WAVE / 2; m >= 1; m >>= 1) {
    num += __shfl_xor(num, m);
    pr += __shfl_xor(pr, m);
  }
  if (lane == 0) { rn[wave] = num; rp[wave] = pr; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long a = 0;
    double b = 0.0;
#pragma unroll
    for (int w = 0; w < FIN_THREADS / WAVE; ++w) { a += rn[w]; b += rp[w]; }
    const bool ok = P > 0 && N > 0;
    out[0] = ok ? ratio_rn(a, 2ull * (unsigned long long)P * (unsigned long long)N) : 0.0;
    out[1] = ok ? b : 0.0;
  }
}

// ---- workspace layout ----------------------------------------------------------------------------------------------------
// one tile-aligned block length for both arrays, so that together they fill RS_GRID blocks
inline long long sort_per(long long n_pos, long long n_neg) {
  return cdiv64(cdiv64(n_pos + n_neg > 0 ? n_pos + n_neg : 1, RS_GRID), RS_TILE) * RS_TILE;
}
inline int sort_blocks(long long n, long long per) { return (int)cdiv64(n, per); }
struct CurveShape { long long per; int blocks; };
inline CurveShape curve_shape(long long p) {
  if (p <= 0) return {1, 0};
  long long b = cdiv64(p, CV_THREADS);
  if (b > CV_MAX_BLOCKS) b = CV_MAX_BLOCKS;
  const long long per = cdiv64(p, b);
  return {per, (int)cdiv64(p, per)};
}
inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

struct Layout { size_t alt_pos, alt_neg, tab_pos, tab_neg, tot, pnum, ppr, total; };
constexpr size_t TOT_BYTES = 4 * 2 * 256 * 4;          // [pass][array][digit]
inline Layout layout(long long n_pos, long long n_neg) {
  Layout L;
  size_t o = 0;
  const long long per = sort_per(n_pos, n_neg);
  L.alt_pos = o; o += up16((size_t)n_pos * 4);
  L.alt_neg = o; o += up16((size_t)n_neg * 4);
  L.tab_pos = o; o += up16((size_t)256 * sort_blocks(n_pos, per) * 4);
  L.tab_neg = o; o += up16((size_t)256 * sort_blocks(n_neg, per) * 4);
  L.tot = o; o += TOT_BYTES;
  L.pnum = o; o += up16((size_t)CV_MAX_BLOCKS * 8);
  L.ppr = o; o += up16((size_t)CV_MAX_BLOCKS * 8);
  L.total = o;
  return L;
}

inline bool supported(long long n_pos, long long n_neg) {
  return n_pos >= 0 && n_neg >= 0 && n_pos + n_neg < (1LL << 31);
}
inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" size_t unet_rank_auc_workspace(int64_t n_pos, int64_t n_neg) {
  if (!supported(n_pos, n_neg)) return 0;
  return layout(n_pos, n_neg).total;
}

extern "C" int32_t unet_rank_auc_append(const float* pred, const float* truth, const uint8_t* select, int64_t n_images,
                                        int64_t per_image, uint32_t* keys, int64_t capacity, int64_t* counts,
                                        void* stream) {
  UNET_REQUIRE(pred && truth && keys && counts, UNET_ERR_BAD_ARG, "unet_rank_auc_append: null pointer");
  UNET_REQUIRE(n_images > 0 && n_images < 65536 && per_image > 0 && capacity > 0, UNET_ERR_BAD_ARG,
               "unet_rank_auc_append: n_images=%lld per_image=%lld capacity=%lld", (long long)n_images,
               (long long)per_image, (long long)capacity);
  hipStream_t s = (hipStream_t)stream;
  const bool vec = per_image % 4 == 0 && aligned(pred, 16) && aligned(truth, 16);
  const long long units = vec ? per_image / 4 : per_image;
  const int bpi = append_bpi(n_images, units);
  AppendParams A{pred, truth, select, (long long)per_image, bpi, keys, (long long)capacity,
                 (unsigned long long*)counts};
  ProfScope prof(UNET_K_OTHER, 0.0, s, "rank_auc_append", (double)n_images * per_image * 8.0);
  if (vec) hipLaunchKernelGGL(rank_auc_append<4>, dim3(bpi, (unsigned)n_images), dim3(AP_THREADS), 0, s, A);
  else hipLaunchKernelGGL(rank_auc_append<1>, dim3(bpi, (unsigned)n_images), dim3(AP_THREADS), 0, s, A);
  return unet_check_launch("rank_auc_append");
}

extern "C" int32_t unet_rank_auc(uint32_t* pos_keys, int64_t n_pos, uint32_t* neg_keys, int64_t n_neg, double* out,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  UNET_REQUIRE(out && workspace && (pos_keys || n_pos == 0) && (neg_keys || n_neg == 0), UNET_ERR_BAD_ARG,
               "unet_rank_auc: null pointer");
  UNET_REQUIRE(n_pos >= 0 && n_neg >= 0, UNET_ERR_BAD_ARG, "unet_rank_auc: negative count");
  UNET_REQUIRE(supported(n_pos, n_neg), UNET_ERR_UNSUPPORTED,
               "unet_rank_auc: n_pos + n_neg = %lld (at most 2^31 - 1 keys)", (long long)(n_pos + n_neg));
  const Layout L = layout(n_pos, n_neg);
  UNET_REQUIRE(workspace_bytes >= L.total && aligned(workspace, 16), UNET_ERR_WORKSPACE,
               "unet_rank_auc: workspace too small or misaligned");
  UNET_REQUIRE(aligned(pos_keys, 16) && aligned(neg_keys, 16), UNET_ERR_BAD_ARG,
               "unet_rank_auc: key arrays must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  unsigned long long* pnum = (unsigned long long*)(ws + L.pnum);
  double* ppr = (double*)(ws + L.ppr);
  const bool ok = n_pos > 0 && n_neg > 0;              // else only the finalize runs: 0 / 0
  const CurveShape cv = curve_shape(ok ? n_pos : 0);
  if (ok) {
    const long long per = sort_per(n_pos, n_neg);
    const int bp = sort_blocks(n_pos, per), bn = sort_blocks(n_neg, per);
    uint32_t* buf[2][2] = {{pos_keys, (uint32_t*)(ws + L.alt_pos)}, {neg_keys, (uint32_t*)(ws + L.alt_neg)}};
    uint32_t* tot = (uint32_t*)(ws + L.tot);
    const dim3 grid(bp + bn);
    ProfScope prof(UNET_K_OTHER, 0.0, s, "radix_scatter", (double)(n_pos + n_neg) * 4 * 4 * 3);
    UNET_REQUIRE(hipMemsetAsync(tot, 0, TOT_BYTES, s) == hipSuccess, UNET_ERR_LAUNCH, "unet_rank_auc: memset failed");
    for (int pass = 0; pass < 4; ++pass) {             // an even number of passes: the result is back in the input
      const int a = pass & 1;
      SortParams P{{{buf[0][a], buf[0][a ^ 1], n_pos, per, bp, (uint32_t*)(ws + L.tab_pos), tot + (2 * pass) * 256},
                    {buf[1][a], buf[1][a ^ 1], n_neg, per, bn, (uint32_t*)(ws + L.tab_neg), tot + (2 * pass + 1) * 256}},
                   8 * pass};
      hipLaunchKernelGGL(radix_hist, grid, dim3(RS_THREADS), 0, s, P);
      int32_t rc = unet_check_launch("radix_hist");
      if (rc) return rc;
      hipLaunchKernelGGL(radix_scan, dim3(256, 2), dim3(SCAN_THREADS), 0, s, P);
      rc = unet_check_launch("radix_scan");
      if (rc) return rc;
      hipLaunchKernelGGL(radix_scatter, grid, dim3(RS_THREADS), 0, s, P);
      rc = unet_check_launch("radix_scatter");
      if (rc) return rc;
    }
  }
  ProfScope prof(UNET_K_OTHER, 0.0, s, "auc_curve", (double)(n_pos + n_neg) * 4);
  if (ok) {
    hipLaunchKernelGGL(auc_curve, dim3(cv.blocks), dim3(CV_THREADS), 0, s, (const uint32_t*)pos_keys, (long long)n_pos,
                       (const uint32_t*)neg_keys, (long long)n_neg, cv.per, pnum, ppr);
    const int32_t rc = unet_check_launch("auc_curve");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(auc_finalize, dim3(1), dim3(FIN_THREADS), 0, s, (const unsigned long long*)pnum,
                     (const double*)ppr, cv.blocks, (long long)n_pos, (long long)n_neg, out);
  return unet_check_launch("auc_finalize");
}
