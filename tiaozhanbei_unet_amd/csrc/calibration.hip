// Calibration of the per-pixel confidence of a segmentation model (no reference counterpart): how well the softmax
// maximum that predict / eval_detection threshold agrees with the accuracy it promises, and the one temperature T that
// minimises the negative log-likelihood of softmax(z / T) on a held-out split.  Two entry points, restated in numpy by
// tests/_calibration_ref.py (the third of that file, the confidence at a temperature, is segvis.hip's seg_confidence
// with SCALED):
//   reliability_histogram  integers only.  Per pixel q = rint(clamp(conf, 0, 1) * 65536) (segpixel.h's conf_q; NaN -> 0),
//                          bin = min(bins - 1, (q * bins) >> 16), and hist[label][bin] += {1, truth == label, q}.  A block
//                          owns ONE tile of RH_THREADS * RH_ITEMS = 4096 consecutive pixels, thread t the pixels t, t +
//                          256, ...: it folds them in registers while the (label, bin) key stays the same (background at a
//                          confidence near 1 is ~99 % of these data sets: one LDS update per thread, not 16 on one word),
//                          commits to the block's LDS copy of the histogram with 32-bit LDS atomics and the block flushes
//                          its non-zero cells with 64-bit integer atomics.  No counter can overflow: a block takes at most
//                          4096 pixels, so an LDS cell is at most 4096 * 65536 = 2^28 < 2^32; the 64-bit cells in memory
//                          hold sums of q <= 65536 per pixel, so they last for 2^47 pixels per cell over all calls.
//   temperature_sweep      one read of the logits gives, for K <= 32 temperatures, the sum over the pixels taken of
//                          logf(sum_j expf(d_j * inv_t[k])) - d_t * inv_t[k], d_j = z_j - z_max.  Per-pixel arithmetic is
//                          fp32 with every product and sum rounded once (this file is built with -ffp-contract=off), sums
//                          are float64.  K * C expf per pixel: the kernel is bound by the vector ALU, not by memory (at
//                          K = 32, C = 4 about 20 x the time its 50 MB would take from HBM; profiles/calibration.txt), and
//                          the library's expf is ~19 instructions of that.  So the class count is a template argument (a
//                          run-time count is predicated, not branched on, by the compiler: all 8 expf for any C), the K
//                          float64 accumulators stay in registers (64 VGPRs; with the 4 x C logits of a lane's unit every
//                          class count fits the 128 VGPRs of 4 waves per SIMD without scratch), a unit's 4 pixels are
//                          handled one after the other in a rolled loop (the unrolled K x C body is ~20 KiB of code at
//                          C = 8) and each class plane is read with one 16-byte load per unit when hw % 4 == 0.
//                          Order of summation, a function of (n, hw, K) alone: a unit is 4 consecutive pixels of one image
//                          (the last one of an image may be short), whichever loads fetch it; block (b, image) owns a fixed
//                          contiguous range of units, thread t its units t, t + 256, ... in order; then a fixed shuffle
//                          tree per wave, the waves in order, one partial per block in the workspace; the finalize kernel
//                          (one block per temperature, one for the counts) sums the partials the same way.  No
//                          floating-point atomics anywhere: two calls on the same input give the same bits.
// A pixel is left out of histogram and sweep alike when its target is ignore_index or outside 0..C-1 (the histogram:
// also when its label byte is >= C; it counts these in `skipped`), and with select == 1 when truth and label are both
// class 0.  The sweep first sets aside every pixel with a non-finite logit (counted[1]), whatever its target.
#include "segpixel.h"

namespace {

using namespace segpx;                                 // MAXC, aligned, conf_q (segpixel.h)
constexpr int MAX_BINS = 64;
constexpr int MAXK = 32;                               // temperatures per sweep
constexpr int RH_THREADS = 256;
constexpr int RH_ITEMS = 16;                           // pixels per thread
constexpr int RH_TILE = RH_THREADS * RH_ITEMS;         // pixels per block: 4096
constexpr int TS_THREADS = 256;
constexpr int TS_WAVES = TS_THREADS / WAVE;
constexpr int TS_MAX_PARTS = 2048;                     // blocks of one sweep, all images together

// ---- reliability histogram ---------------------------------------------------------------------------------------------
struct HistParams {
  const uint8_t* labels; const float* conf; const long long* target;
  long long total;                                     // n * hw
  long long ignore;
  int C, bins, select;
  unsigned long long* hist;                            // [C][bins][3]
  unsigned long long* skipped;
};

// grid = tiles of RH_TILE pixels
__global__ __launch_bounds__(RH_THREADS) void reliability_histogram(const HistParams P) {
  __shared__ unsigned int cell[MAXC * MAX_BINS * 3];   // a block's pixels: at most 4096 * 65536 = 2^28 per cell
  __shared__ unsigned int block_skipped;
  const int cells = P.C * P.bins * 3;
  for (int i = threadIdx.x; i < cells; i += RH_THREADS) cell[i] = 0u;
  if (threadIdx.x == 0) block_skipped = 0u;
  __syncthreads();
  const long long base = (long long)blockIdx.x * RH_TILE + threadIdx.x;
  int lab[RH_ITEMS];
  float cf[RH_ITEMS];
  long long tg[RH_ITEMS];
#pragma unroll
  for (int k = 0; k < RH_ITEMS; ++k) {                 // the loads first
    const long long g = base + (long long)k * RH_THREADS;
    const bool in = g < P.total;
    lab[k] = in ? (int)P.labels[g] : 0;
    cf[k] = in ? P.conf[g] : 0.f;
    tg[k] = in ? P.target[g] : -1;
  }
  unsigned skipped = 0u;
  int key = -1;                                        // the thread's run of pixels of one (label, bin)
  unsigned cnt = 0u, ok = 0u, sq = 0u;                 // at most 16 pixels: sq <= 2^20
#pragma unroll
  for (int k = 0; k < RH_ITEMS; ++k) {
    const long long g = base + (long long)k * RH_THREADS;
    if (g >= P.total) continue;
    const long long t = tg[k];
    const int l = lab[k];
    if (t == P.ignore || t < 0 || t >= P.C || l >= P.C) { ++skipped; continue; }
    if (P.select == 1 && t == 0 && l == 0) continue;
    const unsigned q = conf_q(cf[k]);
    const int bin = min(P.bins - 1, (int)((q * (unsigned)P.bins) >> 16));     // q bins <= 2^22
    const int kk = l * P.bins + bin;                   // < C bins: inside `cell`
    if (kk != key) {
      if (key >= 0) {
        atomicAdd(&cell[3 * key], cnt);
        if (ok) atomicAdd(&cell[3 * key + 1], ok);
        if (sq) atomicAdd(&cell[3 * key + 2], sq);
      }
      key = kk; cnt = ok = sq = 0u;
    }
    ++cnt;
    ok += (t == (long long)l) ? 1u : 0u;
    sq += q;
  }
  if (key >= 0) {
    atomicAdd(&cell[3 * key], cnt);
    if (ok) atomicAdd(&cell[3 * key + 1], ok);
    if (sq) atomicAdd(&cell[3 * key + 2], sq);
  }
#pragma unroll
  for (int m = WAVE / 2; m >= 1; m >>= 1) skipped += __shfl_xor(skipped, m);
  if ((threadIdx.x & (WAVE - 1)) == 0 && skipped) atomicAdd(&block_skipped, skipped);
  __syncthreads();
  for (int i = threadIdx.x; i < cells; i += RH_THREADS) {
    const unsigned v = cell[i];
    if (v) atomicAdd(&P.hist[i], (unsigned long long)v);
  }
  if (threadIdx.x == 0 && block_skipped) atomicAdd(P.skipped, (unsigned long long)block_skipped);
}

// ---- temperature sweep -------------------------------------------------------------------------------------------------
struct SweepParams {
  const float* logits; const long long* target;
  long long hw, ignore;
  int K, select, bpi;                                  // bpi: blocks per image
  float inv_t[MAXK];
  double* pnll;                                        // [n][bpi][K]
  unsigned long long* pcnt;                            // [n][bpi][2]: taken, non-finite
};

inline int sweep_bpi(int n, long long hw) {
  long long b = cdiv64(cdiv64(hw, 4), 2 * TS_THREADS);   // two units per lane where there are that many
  const long long cap = TS_MAX_PARTS / n > 0 ? TS_MAX_PARTS / n : 1;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

// grid (bpi, n).  C is a template argument: with a run-time class count the compiler predicates the class loop instead
// of branching and evaluates all 8 expf for every class count.  VEC: hw % 4 == 0 and 16-byte aligned pointers -- the
// loads differ, the units and their order do not.  The bound asks for the 128 VGPRs of 4 waves per SIMD.
template <bool VEC, int C>
__global__ __launch_bounds__(TS_THREADS, 4) void temperature_sweep(const SweepParams P) {
  __shared__ double red[TS_WAVES][MAXK];
  __shared__ unsigned int redc[TS_WAVES][2];
  const int n = blockIdx.y, b = blockIdx.x, K = P.K;
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const long long units = cdiv64(P.hw, 4);
  const long long per = cdiv64(units, P.bpi);
  const long long u0 = b * per, u1 = min(u0 + per, units);
  const float* x = P.logits + (long long)n * C * P.hw;
  const long long* tg = P.target + (long long)n * P.hw;
  double acc[MAXK];
#pragma unroll
  for (int k = 0; k < MAXK; ++k) acc[k] = 0.0;
  unsigned taken = 0u, bad = 0u;                       // a thread's pixels: far below 2^32 (hw <= 2^31 - 1 over 256 lanes)
  for (long long u = u0 + threadIdx.x; u < u1; u += TS_THREADS) {
    const long long at = 4 * u;
    const int cnt = (int)min(4LL, P.hw - at);          // >= 1: u < units
    f32x4 zv[C];
    long long t0, t1, t2, t3;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if constexpr (VEC) {
        zv[c] = *reinterpret_cast<const f32x4*>(x + c * P.hw + at);
      } else {
        const float* p = x + c * P.hw + at;
        zv[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        zv[c][0] = p[0];
        if (cnt > 1) zv[c][1] = p[1];
        if (cnt > 2) zv[c][2] = p[2];
        if (cnt > 3) zv[c][3] = p[3];
      }
    }
    if constexpr (VEC) {
      typedef __attribute__((ext_vector_type(2))) long long i64x2;
      const i64x2 a = *reinterpret_cast<const i64x2*>(tg + at);
      const i64x2 c2 = *reinterpret_cast<const i64x2*>(tg + at + 2);
      t0 = a[0]; t1 = a[1]; t2 = c2[0]; t3 = c2[1];
    } else {
      t0 = tg[at];
      t1 = cnt > 1 ? tg[at + 1] : -1;
      t2 = cnt > 2 ? tg[at + 2] : -1;
      t3 = cnt > 3 ? tg[at + 3] : -1;
    }
    // the unit's pixels one after the other: element 0 is the current one, the rest move down after each
#pragma unroll 1
    for (int j = 0; j < cnt; ++j) {
      float z[C];
#pragma unroll
      for (int c = 0; c < C; ++c) z[c] = zv[c][0];
      const long long t = t0;
#pragma unroll
      for (int c = 0; c < C; ++c) zv[c] = zv[c].yzwx;
      t0 = t1; t1 = t2; t2 = t3;
      bool fin = true;
#pragma unroll
      for (int c = 0; c < C; ++c) fin = fin && finite_score(z[c]);
      if (!fin) { ++bad; continue; }
      float best = z[0];
      int arg = 0;
#pragma unroll
      for (int c = 1; c < C; ++c)
        if (z[c] > best) { best = z[c]; arg = c; }
      if (t == P.ignore || t < 0 || t >= C) continue;
      if (P.select == 1 && t == 0 && arg == 0) continue;
      ++taken;
      float d[C];
      float dt = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        d[c] = z[c] - best;
        if ((long long)c == t) dt = d[c];
      }
#pragma unroll
      for (int k = 0; k < MAXK; ++k) {
        if (k < K) {                                   // uniform
          const float it = P.inv_t[k];
          float s = 0.f;
#pragma unroll
          for (int c = 0; c < C; ++c) s += expf(d[c] * it);
          acc[k] += (double)(logf(s) - dt * it);
        }
      }
    }
  }
  // fixed-order reductions: shuffle tree within the wave, then the waves in order
#pragma unroll
  for (int k = 0; k < MAXK; ++k) {
    if (k < K) {                                       // uniform
      double v = acc[k];
#pragma unroll
      for (int m = WAVE / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
      if (lane == 0) red[wave][k] = v;
    }
  }
#pragma unroll
  for (int m = WAVE / 2; m >= 1; m >>= 1) {
    taken += __shfl_xor(taken, m);
    bad += __shfl_xor(bad, m);
  }
  if (lane == 0) { redc[wave][0] = taken; redc[wave][1] = bad; }
  __syncthreads();
  const size_t slot = (size_t)n * P.bpi + b;
  if ((int)threadIdx.x < K) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < TS_WAVES; ++w) s += red[w][threadIdx.x];
    P.pnll[slot * K + threadIdx.x] = s;
  }
  if (threadIdx.x < 2) {
    unsigned long long s = 0ull;
#pragma unroll
    for (int w = 0; w < TS_WAVES; ++w) s += redc[w][threadIdx.x];
    P.pcnt[slot * 2 + threadIdx.x] = s;
  }
}

// grid K + 1: block k < K sums the partials of temperature k, block K the two counts; both ADD to their outputs (one
// writer per word, ordered on the stream: no atomics)
__global__ __launch_bounds__(TS_THREADS) void temperature_sweep_finalize(const double* __restrict__ pnll,
                                                                          const unsigned long long* __restrict__ pcnt,
                                                                          int K, int parts, double* __restrict__ nll,
                                                                          unsigned long long* __restrict__ counted) {
  __shared__ double r[TS_WAVES];
  __shared__ unsigned long long rc[TS_WAVES][2];
  const int k = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  if (k < K) {
    double a = 0.0;
    for (int p = tid; p < parts; p += TS_THREADS) a += pnll[(size_t)p * K + k];
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) a += __shfl_xor(a, m);
    if (lane == 0) r[wave] = a;
    __syncthreads();
    if (tid == 0) {
      double s = 0.0;
#pragma unroll
      for (int w = 0; w < TS_WAVES; ++w) s += r[w];
      nll[k] += s;
    }
  } else {
    unsigned long long a = 0ull, c = 0ull;
    for (int p = tid; p < parts; p += TS_THREADS) { a += pcnt[2 * (size_t)p]; c += pcnt[2 * (size_t)p + 1]; }
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) { a += __shfl_xor(a, m); c += __shfl_xor(c, m); }
    if (lane == 0) { rc[wave][0] = a; rc[wave][1] = c; }
    __syncthreads();
    if (tid < 2) {
      unsigned long long s = 0ull;
#pragma unroll
      for (int w = 0; w < TS_WAVES; ++w) s += rc[w][tid];
      counted[tid] += s;
    }
  }
}

template <int C>
void launch_sweep_c(bool vec, dim3 grid, hipStream_t s, const SweepParams& P) {
  if (vec) hipLaunchKernelGGL((temperature_sweep<true, C>), grid, dim3(TS_THREADS), 0, s, P);
  else hipLaunchKernelGGL((temperature_sweep<false, C>), grid, dim3(TS_THREADS), 0, s, P);
}
void launch_sweep(bool vec, int c, dim3 grid, hipStream_t s, const SweepParams& P) {      // c in 2..MAXC: checked by the caller
  switch (c) {
    case 2: return launch_sweep_c<2>(vec, grid, s, P);
    case 3: return launch_sweep_c<3>(vec, grid, s, P);
    case 4: return launch_sweep_c<4>(vec, grid, s, P);
    case 5: return launch_sweep_c<5>(vec, grid, s, P);
    case 6: return launch_sweep_c<6>(vec, grid, s, P);
    case 7: return launch_sweep_c<7>(vec, grid, s, P);
    default: return launch_sweep_c<8>(vec, grid, s, P);
  }
}

inline bool sweep_shape_ok(int64_t n, int64_t hw, int64_t K) {
  return n >= 1 && n < 65536 && hw >= 1 && hw <= (1LL << 31) - 1 && K >= 1 && K <= MAXK;
}

}  // namespace

extern "C" int32_t unet_reliability_histogram(const uint8_t* labels, const float* conf, const int64_t* target, int32_t n,
                                              int64_t hw, int32_t c, int32_t bins, int64_t ignore_index, int32_t select,
                                              uint64_t* hist, uint64_t* skipped, void* stream) {
  const char* who = "unet_reliability_histogram";
  UNET_REQUIRE(labels && conf && target && hist && skipped, UNET_ERR_UNSUPPORTED, "%s: null pointer", who);
  UNET_REQUIRE(n > 0 && hw > 0 && hw <= (1LL << 31) - 1 && c >= 2 && c <= MAXC, UNET_ERR_UNSUPPORTED,
               "%s: n=%d c=%d hw=%lld (2..8 classes, hw <= 2^31 - 1)", who, n, c, (long long)hw);
  UNET_REQUIRE(bins >= 1 && bins <= MAX_BINS && (select == 0 || select == 1), UNET_ERR_UNSUPPORTED,
               "%s: bins=%d select=%d (1..64 bins, select 0 or 1)", who, bins, select);
  hipStream_t s = (hipStream_t)stream;
  const long long total = (long long)n * hw;           // < 2^62; the tiles of 4096 pixels: < 2^31
  const long long tiles = cdiv64(total, RH_TILE);
  UNET_REQUIRE(tiles <= (1LL << 31) - 1, UNET_ERR_UNSUPPORTED, "%s: %lld pixels (fewer than 2^43)", who, total);
  HistParams P{labels, conf, (const long long*)target, total, (long long)ignore_index, c, bins, select,
               (unsigned long long*)hist, (unsigned long long*)skipped};
  ProfScope prof(UNET_K_OTHER, 0.0, s, "reliability_histogram", 13.0 * (double)total);
  hipLaunchKernelGGL(reliability_histogram, dim3((unsigned)tiles), dim3(RH_THREADS), 0, s, P);
  return unet_check_launch("reliability_histogram");
}

extern "C" size_t unet_temperature_sweep_workspace(int32_t n, int64_t hw, int32_t k) {
  if (!sweep_shape_ok(n, hw, k)) return 0;
  const size_t parts = (size_t)n * sweep_bpi(n, hw);
  return parts * ((size_t)k * sizeof(double) + 2 * sizeof(unsigned long long));
}

extern "C" int32_t unet_temperature_sweep(const float* logits, const int64_t* target, int32_t n, int32_t c, int64_t hw,
                                          int64_t ignore_index, int32_t select, const float* inv_t, int32_t k, double* nll,
                                          uint64_t* counted, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "unet_temperature_sweep";
  UNET_REQUIRE(logits && target && inv_t && nll && counted && workspace, UNET_ERR_UNSUPPORTED, "%s: null pointer", who);
  UNET_REQUIRE(sweep_shape_ok(n, hw, k) && c >= 2 && c <= MAXC && (select == 0 || select == 1), UNET_ERR_UNSUPPORTED,
               "%s: n=%d c=%d hw=%lld k=%d select=%d (n < 65536, 2..8 classes, hw <= 2^31 - 1, 1..32 temperatures, select "
               "0 or 1)", who, n, c, (long long)hw, k, select);
  for (int i = 0; i < k; ++i)
    UNET_REQUIRE(inv_t[i] > 0.0f && inv_t[i] <= 3.402823466e38f, UNET_ERR_UNSUPPORTED,
                 "%s: inv_t[%d]=%g is not a finite value > 0", who, i, (double)inv_t[i]);
  UNET_REQUIRE(workspace_bytes >= unet_temperature_sweep_workspace(n, hw, k) && aligned(workspace, 8), UNET_ERR_WORKSPACE,
               "%s: workspace too small or misaligned", who);
  hipStream_t s = (hipStream_t)stream;
  SweepParams P{};
  P.logits = logits; P.target = (const long long*)target;
  P.hw = (long long)hw; P.ignore = (long long)ignore_index;
  P.K = k; P.select = select; P.bpi = sweep_bpi(n, hw);
  for (int i = 0; i < k; ++i) P.inv_t[i] = inv_t[i];
  const size_t parts = (size_t)n * P.bpi;
  P.pnll = (double*)workspace;
  P.pcnt = (unsigned long long*)(P.pnll + parts * k);
  const bool vec = hw % 4 == 0 && aligned(logits, 16) && aligned(target, 16);
  ProfScope prof(UNET_K_OTHER, 0.0, s, "temperature_sweep", (double)n * hw * (4.0 * c + 8.0));
  launch_sweep(vec, c, dim3(P.bpi, n), s, P);
  int32_t rc = unet_check_launch("temperature_sweep");
  if (rc) return rc;
  hipLaunchKernelGGL(temperature_sweep_finalize, dim3(k + 1), dim3(TS_THREADS), 0, s, (const double*)P.pnll,
                     (const unsigned long long*)P.pcnt, k, (int)parts, nll, (unsigned long long*)counted);
  return unet_check_launch("temperature_sweep_finalize");
}
