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
// The per-region-overlap curve (AUPRO) shares the append and the sort: region_auc_append writes the ok pixels as keys and
// the defective ones as (key << 32 | region size) elements (sizes from regions.hip), the three radix kernels are
// templated on the element type, pro_curve / pro_finalize integrate the curve up to the fpr limit (see there).
// No float atomics: the sorted arrays are a function of the pixel multiset and every partition below a function of
// (P, N), so results are bitwise identical whatever the batch split, image order or run.
#include "segpixel.h"

namespace {

using segpx::aligned;
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
// PAIRS (the region curve): truth holds the int32 region sizes of unet_label_regions (positive iff > 0), keys is cap
// 8-byte slots: a positive is the element key << 32 | size from slot 0 up, a negative a uint32 key from the end down
__device__ __forceinline__ uint64_t pair_of(uint32_t key, uint32_t size) { return ((uint64_t)key << 32) | size; }

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

// A block owns a fixed unit range of one image and walks it twice: the first walk counts its positives, negatives and
// non-finite scores (one atomicAdd per class for the whole block reserves its output ranges: a per-wave atomic on
// one address serialised the whole pass), the second walks the same units in the same lane order and writes the
// keys, ranked by ballot within each wave from the wave's base.  The second read mostly hits the caches.
template <int V, bool PAIRS>
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
      const bool fin = finite_score(x[j]), pos = PAIRS ? __float_as_int(y[j]) > 0 : y[j] > 0.5f;
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
      const bool fin = in && finite_score(x[j]), pos = in && (PAIRS ? __float_as_int(y[j]) > 0 : y[j] > 0.5f);
      const unsigned long long bp = __ballot(fin && pos), bn = __ballot(fin && !pos);
      if (fin && pos) {
        const unsigned long long i = pbase + __popcll(bp & lower);
        if (i < (unsigned long long)A.cap) {
          if constexpr (PAIRS) reinterpret_cast<uint64_t*>(A.keys)[i] = pair_of(score_key(x[j]), __float_as_uint(y[j]));
          else A.keys[i] = score_key(x[j]);
        }
      } else if (fin) {
        const unsigned long long i = nbase + __popcll(bn & lower);
        constexpr int SLOT = PAIRS ? 2 : 1;             // uint32 entries per slot
        if (i < (unsigned long long)(SLOT * A.cap)) A.keys[SLOT * A.cap - 1 - (long long)i] = score_key(x[j]);
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
// T: uint32_t keys, or uint64_t (key << 32 | payload) elements sorted on all their bits
template <typename T>
struct SortSegT {
  const T* src; T* dst;
  long long n, per;                                    // per: keys per block, a multiple of RS_TILE
  int blocks;
  uint32_t* table;                                     // [256][blocks]: digit counts, then exclusive offsets
  uint32_t* tot;                                       // [256] keys per digit in this pass (zeroed by the caller)
};
template <typename T>
struct SortParamsT { SortSegT<T> s[2]; int shift; };

template <typename T>
__device__ __forceinline__ int seg_of(const SortParamsT<T>& P, int& lb) {
  lb = blockIdx.x;
  if (lb < P.s[0].blocks) return 0;
  lb -= P.s[0].blocks;
  return 1;
}

template <typename T>
__global__ __launch_bounds__(RS_THREADS) void radix_hist(const SortParamsT<T> P) {
  __shared__ uint32_t h[RS_WAVES][256];
  constexpr int VEC = 16 / sizeof(T);                  // elements of a 16-byte load
  int lb;
  const SortSegT<T> S = P.s[seg_of(P, lb)];
  const int wave = threadIdx.x / WAVE;
  for (int i = threadIdx.x; i < RS_WAVES * 256; i += RS_THREADS) (&h[0][0])[i] = 0;
  __syncthreads();
  const long long start = lb * S.per, end = min(start + S.per, S.n);
  for (long long i = start + VEC * threadIdx.x; i < end; i += VEC * RS_THREADS) {   // start is 16-byte aligned
    if (i + VEC <= end) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(S.src + i);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        T k;
        if constexpr (sizeof(T) == 8) k = ((T)v[2 * j + 1] << 32) | v[2 * j]; else k = v[j];
        atomicAdd(&h[wave][(uint32_t)(k >> P.shift) & 255u], 1u);
      }
    } else {
      for (long long q = i; q < end; ++q) atomicAdd(&h[wave][(uint32_t)(S.src[q] >> P.shift) & 255u], 1u);
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
template <typename T>
__global__ __launch_bounds__(SCAN_THREADS) void radix_scan(const SortParamsT<T> P) {
  __shared__ uint32_t red[SCAN_THREADS / WAVE], wsum[SCAN_THREADS / WAVE];
  const SortSegT<T> S = P.s[blockIdx.y];
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
template <typename T>
__global__ __launch_bounds__(RS_THREADS) void radix_scatter(const SortParamsT<T> P) {
  __shared__ uint16_t cnt[RS_ITEMS][RS_WAVES][256];    // per (sub-tile, wave) digit counts; zero between tiles
  __shared__ uint32_t off[RS_ITEMS][RS_WAVES][256];    // their global start offsets
  __shared__ uint32_t run[256];                        // next free position of each digit in this block's output
  int lb;
  const SortSegT<T> S = P.s[seg_of(P, lb)];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE, tid = threadIdx.x;
  const unsigned long long lower = (1ull << lane) - 1ull;
  for (int i = tid; i < RS_ITEMS * RS_WAVES * 256; i += RS_THREADS) (&cnt[0][0][0])[i] = 0;
  run[tid] = S.table[(size_t)tid * S.blocks + lb];
  __syncthreads();
  const long long start = lb * S.per, end = min(start + S.per, S.n);
  for (long long t0 = start; t0 < end; t0 += RS_TILE) {
    T k[RS_ITEMS];
    int dig[RS_ITEMS], rank[RS_ITEMS];
#pragma unroll
    for (int j = 0; j < RS_ITEMS; ++j) {
      const long long i = t0 + j * RS_THREADS + tid;
      k[j] = i < end ? S.src[i] : (T)0;
    }
#pragma unroll
    for (int j = 0; j < RS_ITEMS; ++j) {
      const bool valid = t0 + j * RS_THREADS + tid < end;
      const int d = (int)((uint32_t)(k[j] >> P.shift) & 255u);
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
template <typename T>
__device__ __forceinline__ long long lower_bound(const T* a, long long lo, long long hi, T v) {
  while (lo < hi) {
    const long long m = lo + ((hi - lo) >> 1);
    if (a[m] < v) lo = m + 1; else hi = m;
  }
  return lo;
}
template <typename T>
__device__ __forceinline__ long long upper_bound(const T* a, long long lo, long long hi, T v) {
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

// ---- per-region-overlap curve ----------------------------------------------------------------------------------------------
// pos: (key << 32 | region size) elements sorted on all 64 bits, neg: sorted keys of the ok pixels.  Walking the scores
// downwards, a defective pixel of value v and region size s lifts the curve by 1 / (s R) along the fpr interval
// [x0, x1] = [#neg > v, #neg >= v] / N, so the area below the curve over [0, L] is the sum over the pixels of
//   1 / (s R) * (L - (x0 + x1) / 2)            x1 <= L
//   1 / (s R) * (L - x0)^2 / (2 (x1 - x0))     x0 < L < x1   (the segment that crosses the limit, cut at it)
// and nothing for x0 >= L.  One lane per run of equal elements (count / s, one rounding); the comparisons with L are
// exact: kfloor = floor(L N), kceil = ceil(L N) from the host.  1 / (R L) is applied once, in pro_finalize.
struct ProParams {
  const uint64_t* pos; long long P;
  const uint32_t* neg; long long N;
  long long per, kfloor, kceil;
  double L;
  double* parea; double* ppro;
};

__global__ __launch_bounds__(CV_THREADS) void pro_curve(const ProParams A) {
  __shared__ double ra[CV_THREADS / WAVE], rp[CV_THREADS / WAVE];
  __shared__ long long nrange[2];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const long long start = blockIdx.x * A.per, end = min(start + A.per, A.P);
  const uint32_t vmax = (uint32_t)(A.pos[end - 1] >> 32);
  // a value below the kceil-th largest ok key has x0 >= L: a block of such values has nothing to add (block-uniform)
  if (vmax < A.neg[A.N - A.kceil]) {
    if (threadIdx.x == 0) { A.parea[blockIdx.x] = 0.0; A.ppro[blockIdx.x] = 0.0; }
    return;
  }
  if (threadIdx.x == 0) {
    nrange[0] = lower_bound(A.neg, 0, A.N, (uint32_t)(A.pos[start] >> 32));
    nrange[1] = upper_bound(A.neg, nrange[0], A.N, vmax);
  }
  __syncthreads();
  const long long nlo = nrange[0], nhi = nrange[1];
  double area = 0.0, pro = 0.0;
  for (long long i = start + threadIdx.x; i < end; i += CV_THREADS) {
    const uint64_t el = A.pos[i];
    if (i > 0 && A.pos[i - 1] == el) continue;         // not the head of its run
    long long last = i, probe = i + 1, step = 1;
    while (probe < A.P && A.pos[probe] == el) { last = probe; probe = last + step; step <<= 1; }
    const long long e = upper_bound(A.pos, last + 1, min(probe, A.P), el);
    const uint32_t v = (uint32_t)(el >> 32);
    const long long lo = lower_bound(A.neg, nlo, nhi, v);
    const long long hi = upper_bound(A.neg, lo, nhi, v);
    const long long c0 = A.N - hi, c1 = A.N - lo;      // ok pixels above v, at or above v
    if (c0 >= A.kceil) continue;
    const double w = (double)(e - i) / (double)(uint32_t)el;
    if (c1 <= A.kfloor) {
      area += w * (A.L - (double)(c0 + c1) / (2.0 * (double)A.N));
      pro += w;
    } else {
      const double t = A.L * (double)A.N - (double)c0, d = (double)(c1 - c0);
      area += w * (t * t / (2.0 * (double)A.N * d));
      pro += w * (t / d);
    }
  }
#pragma unroll
  for (int m = WAVE / 2; m >= 1; m >>= 1) {
    area += __shfl_xor(area, m);
    pro += __shfl_xor(pro, m);
  }
  if (lane == 0) { ra[wave] = area; rp[wave] = pro; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int w = 0; w < CV_THREADS / WAVE; ++w) { a += ra[w]; b += rp[w]; }
    A.parea[blockIdx.x] = a;
    A.ppro[blockIdx.x] = b;
  }
}

__global__ __launch_bounds__(FIN_THREADS) void pro_finalize(const double* __restrict__ parea,
                                                            const double* __restrict__ ppro, int parts, long long R,
                                                            double L, double* __restrict__ out) {
  __shared__ double ra[FIN_THREADS / WAVE], rp[FIN_THREADS / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  double area = 0.0, pro = 0.0;
  for (int b = threadIdx.x; b < parts; b += FIN_THREADS) { area += parea[b]; pro += ppro[b]; }
#pragma unroll
  for (int m = WAVE / 2; m >= 1; m >>= 1) {
    area += __shfl_xor(area, m);
    pro += __shfl_xor(pro, m);
  }
  if (lane == 0) { ra[wave] = area; rp[wave] = pro; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int w = 0; w < FIN_THREADS / WAVE; ++w) { a += ra[w]; b += rp[w]; }
    out[0] = parts > 0 ? a / ((double)R * L) : 0.0;
    out[1] = parts > 0 ? b / (double)R : 0.0;
  }
}

// floor and ceil of L N, exactly: L = m 2^(e - 53) with a 53-bit integer m; 0 < L <= 1, 0 < N < 2^31
inline void limit_ranks(double L, long long N, long long& fl, long long& ce) {
  int e;
  const double f = frexp(L, &e);
  const unsigned __int128 prod = (unsigned __int128)(unsigned long long)ldexp(f, 53) * (unsigned long long)N;
  const int sh = 53 - e;                               // >= 52; prod < 2^84
  if (sh >= 96) { fl = 0; ce = 1; return; }
  fl = (long long)(prod >> sh);
  ce = fl + ((prod & (((unsigned __int128)1 << sh) - 1)) != 0);
}

// one digit of the sort: histogram, scan, scatter
template <typename T>
int32_t sort_pass(const SortParamsT<T>& P, dim3 grid, hipStream_t s) {
  hipLaunchKernelGGL(radix_hist<T>, grid, dim3(RS_THREADS), 0, s, P);
  int32_t rc = unet_check_launch("radix_hist");
  if (rc) return rc;
  hipLaunchKernelGGL(radix_scan<T>, dim3(256, 2), dim3(SCAN_THREADS), 0, s, P);
  rc = unet_check_launch("radix_scan");
  if (rc) return rc;
  hipLaunchKernelGGL(radix_scatter<T>, grid, dim3(RS_THREADS), 0, s, P);
  return unet_check_launch("radix_scatter");
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

constexpr int PAIR_PASSES = 8;                         // at most: 4 digits of the size, 4 of the key
struct RegionLayout { size_t alt_pos, alt_neg, tab_pos, tab_neg, tot, parea, ppro, total; };
inline RegionLayout region_layout(long long n_pos, long long n_neg) {
  RegionLayout L;
  size_t o = 0;
  L.alt_pos = o; o += up16((size_t)n_pos * 8);
  L.alt_neg = o; o += up16((size_t)n_neg * 4);
  L.tab_pos = o; o += up16((size_t)256 * sort_blocks(n_pos, sort_per(n_pos, 0)) * 4);
  L.tab_neg = o; o += up16((size_t)256 * sort_blocks(n_neg, sort_per(0, n_neg)) * 4);
  L.tot = o; o += (size_t)(PAIR_PASSES + 4) * 256 * 4;
  L.parea = o; o += up16((size_t)CV_MAX_BLOCKS * 8);
  L.ppro = o; o += up16((size_t)CV_MAX_BLOCKS * 8);
  L.total = o;
  return L;
}

inline bool supported(long long n_pos, long long n_neg) {
  return n_pos >= 0 && n_neg >= 0 && n_pos + n_neg < (1LL << 31);
}

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
  if (vec) hipLaunchKernelGGL((rank_auc_append<4, false>), dim3(bpi, (unsigned)n_images), dim3(AP_THREADS), 0, s, A);
  else hipLaunchKernelGGL((rank_auc_append<1, false>), dim3(bpi, (unsigned)n_images), dim3(AP_THREADS), 0, s, A);
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
      SortParamsT<uint32_t> P{
          {{buf[0][a], buf[0][a ^ 1], n_pos, per, bp, (uint32_t*)(ws + L.tab_pos), tot + (2 * pass) * 256},
           {buf[1][a], buf[1][a ^ 1], n_neg, per, bn, (uint32_t*)(ws + L.tab_neg), tot + (2 * pass + 1) * 256}},
          8 * pass};
      const int32_t rc = sort_pass(P, grid, s);
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

extern "C" size_t unet_region_auc_workspace(int64_t n_pos, int64_t n_neg) {
  if (!supported(n_pos, n_neg)) return 0;
  return region_layout(n_pos, n_neg).total;
}

extern "C" int32_t unet_region_auc_append(const float* pred, const int32_t* sizes, const uint8_t* select,
                                          int64_t n_images, int64_t per_image, void* slots, int64_t capacity,
                                          int64_t* counts, void* stream) {
  UNET_REQUIRE(pred && sizes && slots && counts, UNET_ERR_BAD_ARG, "unet_region_auc_append: null pointer");
  UNET_REQUIRE(n_images > 0 && n_images < 65536 && per_image > 0 && capacity > 0, UNET_ERR_BAD_ARG,
               "unet_region_auc_append: n_images=%lld per_image=%lld capacity=%lld", (long long)n_images,
               (long long)per_image, (long long)capacity);
  UNET_REQUIRE(aligned(slots, 8), UNET_ERR_BAD_ARG, "unet_region_auc_append: slots must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const bool vec = per_image % 4 == 0 && aligned(pred, 16) && aligned(sizes, 16);
  const long long units = vec ? per_image / 4 : per_image;
  const int bpi = append_bpi(n_images, units);
  AppendParams A{pred, (const float*)sizes, select, (long long)per_image, bpi, (uint32_t*)slots, (long long)capacity,
                 (unsigned long long*)counts};
  ProfScope prof(UNET_K_OTHER, 0.0, s, "region_auc_append", (double)n_images * per_image * 8.0);
  if (vec) hipLaunchKernelGGL((rank_auc_append<4, true>), dim3(bpi, (unsigned)n_images), dim3(AP_THREADS), 0, s, A);
  else hipLaunchKernelGGL((rank_auc_append<1, true>), dim3(bpi, (unsigned)n_images), dim3(AP_THREADS), 0, s, A);
  return unet_check_launch("region_auc_append");
}

extern "C" int32_t unet_region_auc(uint64_t* pos_pairs, int64_t n_pos, uint32_t* neg_keys, int64_t n_neg,
                                   int64_t regions, int64_t max_region, double fpr_limit, double* out, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  UNET_REQUIRE(out && workspace && (pos_pairs || n_pos == 0) && (neg_keys || n_neg == 0), UNET_ERR_BAD_ARG,
               "unet_region_auc: null pointer");
  UNET_REQUIRE(n_pos >= 0 && n_neg >= 0 && regions >= 0 && regions <= n_pos, UNET_ERR_BAD_ARG,
               "unet_region_auc: n_pos=%lld n_neg=%lld regions=%lld", (long long)n_pos, (long long)n_neg,
               (long long)regions);
  UNET_REQUIRE(fpr_limit > 0.0 && fpr_limit <= 1.0, UNET_ERR_BAD_ARG, "unet_region_auc: fpr_limit=%g is not in (0, 1]",
               fpr_limit);
  UNET_REQUIRE(max_region >= 1 && max_region < (1LL << 31), UNET_ERR_BAD_ARG, "unet_region_auc: max_region=%lld",
               (long long)max_region);
  UNET_REQUIRE(supported(n_pos, n_neg), UNET_ERR_UNSUPPORTED,
               "unet_region_auc: n_pos + n_neg = %lld (at most 2^31 - 1 pixels)", (long long)(n_pos + n_neg));
  const RegionLayout L = region_layout(n_pos, n_neg);
  UNET_REQUIRE(workspace_bytes >= L.total && aligned(workspace, 16), UNET_ERR_WORKSPACE,
               "unet_region_auc: workspace too small or misaligned");
  UNET_REQUIRE(aligned(pos_pairs, 16) && aligned(neg_keys, 16), UNET_ERR_BAD_ARG,
               "unet_region_auc: element arrays must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  double* parea = (double*)(ws + L.parea);
  double* ppro = (double*)(ws + L.ppro);
  const bool ok = n_pos > 0 && n_neg > 0 && regions > 0;   // else only the finalize runs: 0 / 0
  const CurveShape cv = curve_shape(ok ? n_pos : 0);
  if (ok) {
    uint32_t* tot = (uint32_t*)(ws + L.tot);
    ProfScope prof(UNET_K_OTHER, 0.0, s, "radix_scatter", 0.0);
    UNET_REQUIRE(hipMemsetAsync(tot, 0, (size_t)(PAIR_PASSES + 4) * 256 * 4, s) == hipSuccess, UNET_ERR_LAUNCH,
                 "unet_region_auc: memset failed");
    // the pairs on every bit that can differ: the digits of the size below max_region, then the key's four
    int size_digits = 1;
    while (size_digits < 4 && (max_region >> (8 * size_digits)) != 0) ++size_digits;
    uint64_t* pbuf[2] = {pos_pairs, (uint64_t*)(ws + L.alt_pos)};
    const long long per_p = sort_per(n_pos, 0);
    const int bp = sort_blocks(n_pos, per_p);
    int at = 0;
    for (int pass = 0; pass < size_digits + 4; ++pass, at ^= 1) {
      SortParamsT<uint64_t> P{{{pbuf[at], pbuf[at ^ 1], n_pos, per_p, bp, (uint32_t*)(ws + L.tab_pos), tot + pass * 256},
                               {nullptr, nullptr, 0, per_p, 0, nullptr, nullptr}},
                              pass < size_digits ? 8 * pass : 32 + 8 * (pass - size_digits)};
      const int32_t rc = sort_pass(P, dim3(bp), s);
      if (rc) return rc;
    }
    uint32_t* nbuf[2] = {neg_keys, (uint32_t*)(ws + L.alt_neg)};
    const long long per_n = sort_per(0, n_neg);
    const int bn = sort_blocks(n_neg, per_n);
    for (int pass = 0; pass < 4; ++pass) {
      const int a = pass & 1;
      SortParamsT<uint32_t> P{{{nbuf[a], nbuf[a ^ 1], n_neg, per_n, bn, (uint32_t*)(ws + L.tab_neg),
                                tot + (PAIR_PASSES + pass) * 256},
                               {nullptr, nullptr, 0, per_n, 0, nullptr, nullptr}},
                              8 * pass};
      const int32_t rc = sort_pass(P, dim3(bn), s);
      if (rc) return rc;
    }
    ProParams C{pbuf[at], (long long)n_pos, neg_keys, (long long)n_neg, cv.per, 0, 0, fpr_limit, parea, ppro};
    limit_ranks(fpr_limit, n_neg, C.kfloor, C.kceil);
    hipLaunchKernelGGL(pro_curve, dim3(cv.blocks), dim3(CV_THREADS), 0, s, C);
    const int32_t rc = unet_check_launch("pro_curve");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(pro_finalize, dim3(1), dim3(FIN_THREADS), 0, s, (const double*)parea, (const double*)ppro,
                     cv.blocks, (long long)regions, fpr_limit, out);
  return unet_check_launch("pro_finalize");
}
