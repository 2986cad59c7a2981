// Per-image evaluation statistics of the Gear / Kolektor evaluation CLIs:
//   compute_prediction_stats   reference visualize.py:239-257 (softmax, argmax, accuracy, max-probability
//                              mean / std, per-class accuracy)
//   SegmentationMetrics.update reference src/metrics.py:22-45 (the confusion matrix, summed over images)
// The reference copies every logit map to the host for this; here one streaming pass over the fp32 NCHW logits
// produces, per image, the C x C confusion counts, the fp64 sum and sum of squares of the per-pixel maximum softmax
// probability and, optionally, the uint8 label map.  HBM-bound, no MFMA:
//   seg_stats_kernel     grid (blocks per image, N): a block owns a fixed contiguous pixel range of one image; a lane
//                        handles 4 pixels (one 16-byte read per class plane, a 32-byte target read, one 4-byte label
//                        store) when hw % 4 == 0 and the pointers allow it, else 1.  Confusion counts are aggregated
//                        per wave (ballot over equal (truth, prediction) keys) into a per-wave LDS histogram; the
//                        fp64 sums go through a fixed shuffle tree.  Each block writes its partials to the workspace.
//   seg_stats_finalize   grid N: ordered sums of the block partials -> uint64 confusion, mean and unbiased std.
// No float atomics, no global atomics at all: the pixel -> lane -> block mapping is a function of (n, c, hw) only,
// so results are bitwise identical from run to run.
#include "segpixel.h"

namespace {

using segpx::MAXC;
using segpx::aligned;
constexpr int ST_THREADS = 256;
constexpr int ST_WAVES = ST_THREADS / WAVE;
constexpr int FIN_THREADS = 256;

struct StatsParams {
  const float* logits; const long long* target; unsigned char* labels;
  int C; long long hw; long long ignore;
  int bpi;                               // blocks per image
  double* psum;                          // [N][bpi][2]  sum p, sum p^2
  unsigned int* pcnt;                    // [N][bpi][C*C]
};

// argmax (first maximum, strict >: torch.argmax / seg_confusion_kernel) and the maximum softmax probability
// 1 / (1 + sum_{c != argmax} exp(z_c - z_max)), the exponentials and the sum in fp64
__device__ __forceinline__ int argmax_pmax(const float (&z)[MAXC], int C, double& pmax) {
  float best = z[0];
  int arg = 0;
#pragma unroll
  for (int c = 1; c < MAXC; ++c)
    if (c < C && z[c] > best) { best = z[c]; arg = c; }
  double s = 1.0;
#pragma unroll
  for (int c = 0; c < MAXC; ++c)
    if (c < C && c != arg) s += exp((double)z[c] - (double)best);
  pmax = 1.0 / s;
  return arg;
}

// add one (truth, prediction) key per lane (-1: nothing) to this wave's histogram: one LDS update per distinct key
__device__ __forceinline__ void wave_count(int key, int lane, unsigned int* hist) {
  unsigned long long pending = __ballot(key >= 0);
  while (pending) {
    const int leader = __ffsll((long long)pending) - 1;
    const int k = __shfl(key, leader);
    const unsigned long long same = __ballot(key == k);
    if (lane == leader) hist[k] += (unsigned int)__popcll(same);
    pending &= ~same;
  }
}

template <int V>
__global__ __launch_bounds__(ST_THREADS) void seg_stats_kernel(const StatsParams P) {
  __shared__ unsigned int hist[ST_WAVES][MAXC * MAXC];
  __shared__ double red[ST_WAVES][2];
  const int n = blockIdx.y, b = blockIdx.x, C = P.C;
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  for (int i = threadIdx.x; i < ST_WAVES * MAXC * MAXC; i += ST_THREADS) (&hist[0][0])[i] = 0;
  __syncthreads();

  const long long units = P.hw / V;                        // V divides hw
  const long long per = cdiv64(units, P.bpi);
  const long long u0 = b * per, u1 = min(u0 + per, units);
  const float* x = P.logits + (long long)n * C * P.hw;
  const long long* tg = P.target ? P.target + (long long)n * P.hw : nullptr;
  unsigned char* lab = P.labels ? P.labels + (long long)n * P.hw : nullptr;
  double s1 = 0.0, s2 = 0.0;
  // every lane runs the same trip count (the wave-wide ballots need the whole wave)
  for (long long base = u0; base < u1; base += ST_THREADS) {
    const long long u = base + threadIdx.x;
    const bool in = u < u1;
    float z[V][MAXC];
    long long t[V];
    if (in) {
#pragma unroll
      for (int c = 0; c < MAXC; ++c) {
        if (c < C) {
          if constexpr (V == 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + c * P.hw + 4 * u);
            z[0][c] = v[0]; z[1][c] = v[1]; z[2][c] = v[2]; z[3][c] = v[3];
          } else {
            z[0][c] = x[c * P.hw + u];
          }
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j) z[j][c] = 0.f;
        }
      }
      if (tg) {
        if constexpr (V == 4) {
          typedef __attribute__((ext_vector_type(2))) long long i64x2;
          const i64x2 a = *reinterpret_cast<const i64x2*>(tg + 4 * u);
          const i64x2 c2 = *reinterpret_cast<const i64x2*>(tg + 4 * u + 2);
          t[0] = a[0]; t[1] = a[1]; t[2] = c2[0]; t[3] = c2[1];
        } else {
          t[0] = tg[u];
        }
      }
    }
    int arg[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      arg[j] = 0;
      if (in) {
        double p;
        arg[j] = argmax_pmax(z[j], C, p);
        s1 += p;
        s2 += p * p;
      }
    }
    if (in && lab) {
      if constexpr (V == 4) {
        const unsigned int w = (unsigned)arg[0] | ((unsigned)arg[1] << 8) | ((unsigned)arg[2] << 16) |
                               ((unsigned)arg[3] << 24);
        *reinterpret_cast<unsigned int*>(lab + 4 * u) = w;
      } else {
        lab[u] = (unsigned char)arg[0];
      }
    }
    if (tg) {                                               // wave-uniform
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const bool valid = in && t[j] != P.ignore && t[j] >= 0 && t[j] < C;
        wave_count(valid ? (int)t[j] * C + arg[j] : -1, lane, hist[wave]);
      }
    }
  }

  // fixed-order reductions: shuffle tree within the wave, then the waves in order
#pragma unroll
  for (int m = WAVE / 2; m >= 1; m >>= 1) {
    s1 += __shfl_xor(s1, m);
    s2 += __shfl_xor(s2, m);
  }
  if (lane == 0) { red[wave][0] = s1; red[wave][1] = s2; }
  __syncthreads();
  const size_t slot = (size_t)n * P.bpi + b;
  if (threadIdx.x < 2) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < ST_WAVES; ++w) s += red[w][threadIdx.x];
    P.psum[slot * 2 + threadIdx.x] = s;
  }
  if (threadIdx.x < C * C) {
    unsigned int s = 0;
#pragma unroll
    for (int w = 0; w < ST_WAVES; ++w) s += hist[w][threadIdx.x];
    P.pcnt[slot * C * C + threadIdx.x] = s;
  }
}

// one block per image.  A thread owns blocks b = tid, tid + 256, ... and issues all their loads at once (the partials
// were written from every XCD: each load is a far miss, so a dependent chain of them would dominate); then a fixed
// shuffle tree per quantity within each wave and the waves in order through LDS.
__global__ __launch_bounds__(FIN_THREADS) void seg_stats_finalize(const double* __restrict__ psum,
                                                                  const unsigned int* __restrict__ pcnt, int C, int bpi,
                                                                  long long hw, unsigned long long* __restrict__ cm,
                                                                  double* __restrict__ conf) {
  __shared__ double r[FIN_THREADS / WAVE][2];
  __shared__ unsigned long long rc[FIN_THREADS / WAVE][MAXC * MAXC];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int CC = C * C;
  double a = 0.0, q = 0.0;
  unsigned long long acc[MAXC * MAXC];
#pragma unroll
  for (int i = 0; i < MAXC * MAXC; ++i) acc[i] = 0;
  for (int b = tid; b < bpi; b += FIN_THREADS) {
    const size_t slot = (size_t)n * bpi + b;
    a += psum[2 * slot];
    q += psum[2 * slot + 1];
    if (cm) {
#pragma unroll
      for (int i = 0; i < MAXC * MAXC; ++i)
        if (i < CC) acc[i] += pcnt[slot * CC + i];
    }
  }
#pragma unroll
  for (int m = WAVE / 2; m >= 1; m >>= 1) {
    a += __shfl_xor(a, m);
    q += __shfl_xor(q, m);
  }
  if (lane == 0) { r[wave][0] = a; r[wave][1] = q; }
  if (cm) {
#pragma unroll
    for (int i = 0; i < MAXC * MAXC; ++i) {
      if (i < CC) {                                         // uniform
        unsigned long long v = acc[i];
#pragma unroll
        for (int m = WAVE / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
        if (lane == 0) rc[wave][i] = v;
      }
    }
  }
  __syncthreads();
  if (cm && tid < CC) {
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < FIN_THREADS / WAVE; ++w) s += rc[w][tid];
    cm[(size_t)n * CC + tid] = s;
  }
  if (tid == 0) {
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int w = 0; w < FIN_THREADS / WAVE; ++w) { s1 += r[w][0]; s2 += r[w][1]; }
    const double cnt = (double)hw;
    const double mean = s1 / cnt;
    const double var = (s2 - s1 * mean) / (cnt - 1.0);       // hw == 1: 0 / 0 = NaN, as torch.std
    conf[2 * n] = mean;
    conf[2 * n + 1] = sqrt(var > 0.0 ? var : (var == var ? 0.0 : var));
  }
}

inline int stats_bpi(int n, long long units) {
  long long b = cdiv64(units, 4 * ST_THREADS);           // >= 4 units per lane
  const long long cap = 2048 / n > 0 ? 2048 / n : 1;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace

extern "C" size_t unet_seg_image_stats_workspace(int32_t n, int32_t c, int64_t hw) {
  if (n <= 0 || hw <= 0 || c < 2 || c > MAXC) return 0;
  const int bpi = stats_bpi(n, hw);                        // the scalar layout (V = 1) has the most blocks
  return (size_t)n * bpi * (2 * sizeof(double) + (size_t)c * c * sizeof(unsigned int));
}

extern "C" int32_t unet_seg_image_stats(const float* logits, const int64_t* target, int32_t n, int32_t c, int64_t hw,
                                        int64_t ignore_index, uint8_t* labels, int64_t* confusion, double* conf,
                                        void* workspace, size_t workspace_bytes, void* stream) {
  UNET_REQUIRE(logits && conf && workspace, UNET_ERR_BAD_ARG, "unet_seg_image_stats: null pointer");
  UNET_REQUIRE(n > 0 && hw > 0 && c >= 2 && c <= MAXC, UNET_ERR_UNSUPPORTED,
               "unet_seg_image_stats: n=%d c=%d hw=%lld (2..8 classes)", n, c, (long long)hw);
  UNET_REQUIRE(workspace_bytes >= unet_seg_image_stats_workspace(n, c, hw) && aligned(workspace, 8), UNET_ERR_WORKSPACE,
               "unet_seg_image_stats: workspace too small or misaligned");
  hipStream_t s = (hipStream_t)stream;
  const bool vec = hw % 4 == 0 && aligned(logits, 16) && (!target || aligned(target, 16)) && (!labels || aligned(labels, 4));
  const long long units = vec ? hw / 4 : hw;
  const int bpi = stats_bpi(n, units);
  UNET_REQUIRE(cdiv64(units, bpi) * (vec ? 4 : 1) < (1LL << 32), UNET_ERR_UNSUPPORTED,
               "unet_seg_image_stats: hw=%lld too large for %d images", (long long)hw, n);   // uint32 block counts
  double* psum = (double*)workspace;
  unsigned int* pcnt = (unsigned int*)(psum + (size_t)n * bpi * 2);
  StatsParams P{logits, (const long long*)target, labels, c, (long long)hw, (long long)ignore_index, bpi, psum, pcnt};
  const double bytes = (double)n * hw * (4.0 * c + (target ? 8.0 : 0.0) + (labels ? 1.0 : 0.0));
  ProfScope prof(UNET_K_OTHER, 0.0, s, "seg_stats_kernel", bytes);
  if (vec) hipLaunchKernelGGL(seg_stats_kernel<4>, dim3(bpi, n), dim3(ST_THREADS), 0, s, P);
  else hipLaunchKernelGGL(seg_stats_kernel<1>, dim3(bpi, n), dim3(ST_THREADS), 0, s, P);
  int32_t rc = unet_check_launch("seg_stats_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(seg_stats_finalize, dim3(n), dim3(FIN_THREADS), 0, s, (const double*)psum, (const unsigned int*)pcnt,
                     c, bpi, (long long)hw, target ? (unsigned long long*)confusion : nullptr, conf);
  rc = unet_check_launch("seg_stats_finalize");
  if (rc || !confusion || target) return rc;
  // no target: nothing is counted, the confusion output is all zeros
  return hipMemsetAsync(confusion, 0, (size_t)n * c * c * sizeof(int64_t), s) == hipSuccess ? 0 : UNET_ERR_LAUNCH;
}
