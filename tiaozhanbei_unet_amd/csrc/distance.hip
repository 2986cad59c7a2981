// Exact squared Euclidean distance to class boundaries, and the outline statistics of two label maps that rest on it.
// classes: uint8 [n][h][w]; a pixel has class c iff its value is c with 1 <= c < num_classes.  A pixel of class c is a
// boundary pixel of c iff one of its 4-neighbours INSIDE the frame has another value (the frame edge makes no boundary).
// d2[n][c - 1][y][x] = min (y - y')^2 + (x - x')^2 over the boundary pixels of class c of image n, BOUNDARY_NONE = 1 << 30
// where the image has none.  Integers throughout: the output is a function of the label map alone.
//
// unet_boundary_distance_sq, two launches (the distance separates: min over x' of (x - x')^2 + min over y' of (y - y')^2):
//   edt_column_pass   a thread per column x (a wave's row read is one line), CG classes per thread from one read of the
//                     labels; grid z walks the class groups.  Down the column it keeps, per class, the last boundary row
//                     and writes the distance to it; up the column it reads that back (0 = a boundary), keeps the next
//                     boundary row and writes g^2 = min(down, up)^2, or BOUNDARY_NONE for a column without a boundary.  A
//                     column that saw a boundary of class c raises flag[n][c - 1] (atomicOr on a cleared workspace).
//                     The walk is sequential and latency-bound: both ways it takes COL_ROWS rows at a time, all their
//                     loads issued before the first value is used.
//   edt_row_pass      a workgroup per (row, class, image), in place: the g^2 row goes to LDS (at most 16 KiB), then each
//                     lane takes the outputs x, x + ROW_THREADS, ... and searches x' = x -+ dx outward, best =
//                     min(best, g^2[x'] + dx^2), until dx^2 >= best: nothing farther can win, since g^2 >= 0.  The lanes
//                     of a wave read consecutive LDS words (no bank conflict) and a pixel costs about its distance in
//                     steps.  BOUNDARY_NONE + dx^2 < 2^30 + 2^24 fits int32, so it serves as the pass's infinity.  A
//                     class without a flag keeps the column pass's BOUNDARY_NONE rows and the workgroup returns at once.
//
// unet_boundary_stats, one launch over the pixels of truth and prediction with both d2 maps:
//   boundary_stats    a pixel is a boundary pixel of its class iff its own d2 is 0, so the labels' neighbours are not
//                     read again, and it touches the counters of at most two classes (the truth's, the prediction's).
//                     Counts, fixed-point distance sums and maxima are added in LDS ([classes][fields], 64-bit adds,
//                     32-bit maxima; the pixel counts of a wave whose lanes agree take one add), then every non-zero word
//                     goes to the image's record with one 64-bit atomicAdd / atomicMax.  The pooled histogram has too
//                     many bins for LDS at 32 classes: the lanes of a wave that share a bin are counted with ballots and
//                     one of them adds to the 64-bit bin.  dist_q8 = isqrt(d2 << 16) and the bin isqrt(d2) come from a
//                     double sqrt corrected by integer comparison.  Integer adds and maxima are exact in any order.
// Every loop is counted; a label indexes only after 1 <= v < num_classes has been checked.
#include "unionfind.h"

namespace {

using uf::up16;
typedef unsigned long long u64;

constexpr int NONE = 1 << 30;                          // BOUNDARY_NONE
constexpr int MAX_SIDE = 4096, MAX_CLASSES = 32;
constexpr int COL_THREADS = 64, CG = 4;                // columns per block (one wave: more blocks), classes per thread
constexpr int COL_ROWS = 8;                            // rows of a column in flight
constexpr int ROW_THREADS = 256;
constexpr int ST_THREADS = 256, ST_ITEMS = 8;          // pixels per lane of boundary_stats
constexpr int MAX_TOL = 4, HIST_BINS = 1025;
// record fields (int64): image, class, then SUMS added fields, then the two maxima
enum { F_IMAGE, F_CLASS, F_T_PIXELS, F_P_PIXELS, F_T_BOUNDARY, F_P_BOUNDARY, F_P_NEAR, F_T_NEAR = F_P_NEAR + MAX_TOL,
       F_BAND_INTER = F_T_NEAR + MAX_TOL, F_BAND_UNION, F_P_SUM, F_T_SUM, F_P_MAX, F_T_MAX, FIELDS };
constexpr int SUMS = F_P_MAX - F_T_PIXELS;
static_assert(FIELDS == UNET_BOUNDARY_FIELDS && NONE == UNET_BOUNDARY_NONE, "include/unet_hip.h states both");

struct ColParams {
  const uint8_t* classes; int* d2; int* flag;
  int h, w, C;
};

// grid (w / COL_THREADS, images, class groups)
__global__ __launch_bounds__(COL_THREADS) void edt_column_pass(const ColParams A) {
  const int x = blockIdx.x * COL_THREADS + threadIdx.x;
  if (x >= A.w) return;
  const int n = blockIdx.y, c0 = 1 + blockIdx.z * CG, h = A.h, w = A.w, fg = A.C - 1;
  const long long per = (long long)h * w;
  const uint8_t* __restrict__ m = A.classes + (long long)n * per + x;
  int* out[CG];
  int last[CG];
#pragma unroll
  for (int k = 0; k < CG; ++k) {                       // a class past the last one borrows the group's first plane, unused
    const int c = c0 + k < A.C ? c0 + k : c0;
    out[k] = A.d2 + ((long long)n * fg + (c - 1)) * per + x;
    last[k] = -1;
  }
  // COL_ROWS rows at a time: all their loads are issued before the first is used, so a lane waits once per chunk, not
  // once per row.  A value outside the frame is -1: it differs from nothing.
  int up = -1, cur = m[0];
  for (int y0 = 0; y0 < h; y0 += COL_ROWS) {
    int down[COL_ROWS], left[COL_ROWS], right[COL_ROWS];
#pragma unroll
    for (int j = 0; j < COL_ROWS; ++j) {
      const int y = y0 + j;
      const long long at = (long long)y * w;
      down[j] = y + 1 < h ? m[at + w] : -1;
      left[j] = y < h && x > 0 ? m[at - 1] : -1;
      right[j] = y < h && x + 1 < w ? m[at + 1] : -1;
    }
#pragma unroll
    for (int j = 0; j < COL_ROWS; ++j) {
      const int y = y0 + j;
      if (y >= h) break;
      const long long at = (long long)y * w;
      const bool b = cur >= 1 && cur < A.C && ((left[j] >= 0 && left[j] != cur) || (right[j] >= 0 && right[j] != cur) ||
                                               (up >= 0 && up != cur) || (down[j] >= 0 && down[j] != cur));
#pragma unroll
      for (int k = 0; k < CG; ++k) {
        if (c0 + k >= A.C) continue;
        if (b && cur == c0 + k) last[k] = y;
        out[k][at] = last[k] >= 0 ? y - last[k] : NONE;
      }
      up = cur;
      cur = down[j];
    }
  }
  int next[CG];
#pragma unroll
  for (int k = 0; k < CG; ++k) {
    if (c0 + k < A.C && last[k] >= 0) atomicOr(&A.flag[n * fg + c0 + k - 1], 1);
    next[k] = -1;
  }
  for (int y0 = h - 1; y0 >= 0; y0 -= COL_ROWS) {      // back up: the same chunks of this thread's own stores
    int dd[CG][COL_ROWS];
#pragma unroll
    for (int j = 0; j < COL_ROWS; ++j)
#pragma unroll
      for (int k = 0; k < CG; ++k) dd[k][j] = y0 - j >= 0 && c0 + k < A.C ? out[k][(long long)(y0 - j) * w] : NONE;
#pragma unroll
    for (int j = 0; j < COL_ROWS; ++j) {
      const int y = y0 - j;
      if (y < 0) break;
#pragma unroll
      for (int k = 0; k < CG; ++k) {
        if (c0 + k >= A.C) continue;
        if (dd[k][j] == 0) next[k] = y;
        const int g = next[k] >= 0 ? min(dd[k][j], next[k] - y) : dd[k][j];
        out[k][(long long)y * w] = g >= NONE ? NONE : g * g;      // g <= 4095
      }
    }
  }
}

struct RowParams {
  int* d2; const int* flag;
  int h, w, fg;
};

// grid (rows, foreground classes, images), in place
__global__ __launch_bounds__(ROW_THREADS) void edt_row_pass(const RowParams A) {
  __shared__ int g[MAX_SIDE];
  const int y = blockIdx.x, c = blockIdx.y, n = blockIdx.z, w = A.w;
  if (A.flag[n * A.fg + c] == 0) return;               // block-uniform: every row is BOUNDARY_NONE already
  int* row = A.d2 + (((long long)n * A.fg + c) * A.h + y) * w;
  for (int x = threadIdx.x; x < w; x += ROW_THREADS) g[x] = row[x];
  __syncthreads();
  for (int x = threadIdx.x; x < w; x += ROW_THREADS) {
    int best = g[x];
    const int lim = max(x, w - 1 - x);
    for (int dx = 1; dx <= lim; ++dx) {
      const int q = dx * dx;
      if (q >= best) break;
      if (x - dx >= 0) best = min(best, g[x - dx] + q);
      if (x + dx < w) best = min(best, g[x + dx] + q);
    }
    row[x] = best;
  }
}

struct StatParams {
  const uint8_t* truth; const uint8_t* pred;
  const int* d2t; const int* d2p;
  int C, k, band_sq, image_base;
  int tol_sq[MAX_TOL];
  long long per;
  u64* rec;                                            // [n][C - 1][FIELDS]
  u64* hist;                                           // [C - 1][2][HIST_BINS]
};

// floor(sqrt(v)), v < 2^42: the double is exact, its root rounded once; the comparisons settle the last unit
__device__ __forceinline__ u64 isqrt64(u64 v) {
  u64 r = (u64)sqrt((double)v);
  while (r * r > v) --r;
  while ((r + 1) * (r + 1) <= v) ++r;
  return r;
}

// every lane of the wave calls this; the lanes with `on` that share a bin are counted by one of them
__device__ __forceinline__ void hist_add(u64* hist, bool on, int bin, int lane) {
  u64 pending = __ballot(on);
  while (pending) {                                    // wave-uniform; a round retires at least its leader
    const int first = __ffsll((long long)pending) - 1;
    const int lead = __shfl(bin, first);
    const u64 same = __ballot(on && bin == lead);
    if (lane == first) atomicAdd(&hist[lead], (u64)__popcll(same));
    if (bin == lead) on = false;
    pending &= ~same;
  }
}

// grid (pixels of one image / (ST_THREADS * ST_ITEMS), images)
__global__ __launch_bounds__(ST_THREADS) void boundary_stats(const StatParams A) {
  __shared__ u64 sums[MAX_CLASSES - 1][SUMS];
  __shared__ int maxs[MAX_CLASSES - 1][2];
  const int n = blockIdx.y, fg = A.C - 1, lane = threadIdx.x & (WAVE - 1);
  for (int i = threadIdx.x; i < fg * SUMS; i += ST_THREADS) sums[i / SUMS][i % SUMS] = 0;
  for (int i = threadIdx.x; i < fg * 2; i += ST_THREADS) maxs[i / 2][i % 2] = 0;
  __syncthreads();
  const long long per = A.per;
  const uint8_t* truth = A.truth + (long long)n * per;
  const uint8_t* pred = A.pred + (long long)n * per;
  const int* d2t = A.d2t + (long long)n * fg * per;
  const int* d2p = A.d2p + (long long)n * fg * per;
  const long long block0 = (long long)blockIdx.x * (ST_THREADS * ST_ITEMS);
  for (int it = 0; it < ST_ITEMS; ++it) {              // every lane runs every round (the ballots want that)
    const long long pix = block0 + it * ST_THREADS + threadIdx.x;
    const bool in = pix < per;
    int tv = in ? truth[pix] : 0, pv = in ? pred[pix] : 0;
    if (tv >= A.C) tv = 0;                             // background
    if (pv >= A.C) pv = 0;
    // the pixel counts: one add for a wave whose lanes agree
    const int key = tv << 8 | pv;
    if (__ballot(key != __shfl(key, 0)) == 0ull) {
      if (lane == 0) {
        if (tv) atomicAdd(&sums[tv - 1][F_T_PIXELS - 2], (u64)WAVE);
        if (pv) atomicAdd(&sums[pv - 1][F_P_PIXELS - 2], (u64)WAVE);
      }
    } else {
      if (tv) atomicAdd(&sums[tv - 1][F_T_PIXELS - 2], 1ull);
      if (pv) atomicAdd(&sums[pv - 1][F_P_PIXELS - 2], 1ull);
    }
    int tt = NONE, tp = NONE, pp = NONE, pt = NONE;    // d2 of the truth's class in truth / pred, of the pred's class in pred / truth
    if (tv) tt = d2t[(long long)(tv - 1) * per + pix];
    if (pv) pp = d2p[(long long)(pv - 1) * per + pix];
    const bool tb = tt == 0, pb = pp == 0;             // boundary pixels
    if (tb) tp = d2p[(long long)(tv - 1) * per + pix];
    if (pb) pt = d2t[(long long)(pv - 1) * per + pix];
    // Boundary IoU's bands
    const bool in_t = tt <= A.band_sq, in_p = pp <= A.band_sq;
    if (tv && tv == pv) {
      if (in_t && in_p) atomicAdd(&sums[tv - 1][F_BAND_INTER - 2], 1ull);
      if (in_t || in_p) atomicAdd(&sums[tv - 1][F_BAND_UNION - 2], 1ull);
    } else {
      if (in_t) atomicAdd(&sums[tv - 1][F_BAND_UNION - 2], 1ull);
      if (in_p) atomicAdd(&sums[pv - 1][F_BAND_UNION - 2], 1ull);
    }
    // the outlines: this map's boundary pixels against the other map's distance
    if (tb) atomicAdd(&sums[tv - 1][F_T_BOUNDARY - 2], 1ull);
    if (pb) atomicAdd(&sums[pv - 1][F_P_BOUNDARY - 2], 1ull);
    const bool t_on = tb && tp < NONE, p_on = pb && pt < NONE;
    if (t_on) {
      for (int k = 0; k < A.k; ++k)
        if (tp <= A.tol_sq[k]) atomicAdd(&sums[tv - 1][F_T_NEAR - 2 + k], 1ull);
      atomicAdd(&sums[tv - 1][F_T_SUM - 2], isqrt64((u64)tp << 16));
      atomicMax(&maxs[tv - 1][1], tp);
    }
    if (p_on) {
      for (int k = 0; k < A.k; ++k)
        if (pt <= A.tol_sq[k]) atomicAdd(&sums[pv - 1][F_P_NEAR - 2 + k], 1ull);
      atomicAdd(&sums[pv - 1][F_P_SUM - 2], isqrt64((u64)pt << 16));
      atomicMax(&maxs[pv - 1][0], pt);
    }
    const int p_bin = p_on ? ((pv - 1) * 2 + 0) * HIST_BINS + min((int)isqrt64((u64)pt), HIST_BINS - 1) : 0;
    const int t_bin = t_on ? ((tv - 1) * 2 + 1) * HIST_BINS + min((int)isqrt64((u64)tp), HIST_BINS - 1) : 0;
    hist_add(A.hist, p_on, p_bin, lane);
    hist_add(A.hist, t_on, t_bin, lane);
  }
  __syncthreads();
  u64* rec = A.rec + (long long)n * fg * FIELDS;
  for (int i = threadIdx.x; i < fg * SUMS; i += ST_THREADS) {
    const u64 v = sums[i / SUMS][i % SUMS];
    if (v) atomicAdd(&rec[(i / SUMS) * FIELDS + 2 + i % SUMS], v);
  }
  for (int i = threadIdx.x; i < fg * 2; i += ST_THREADS) {
    const int v = maxs[i / 2][i % 2];
    if (v) atomicMax(&rec[(i / 2) * FIELDS + F_P_MAX + i % 2], (u64)v);
  }
  if (blockIdx.x == 0)
    for (int c = threadIdx.x; c < fg; c += ST_THREADS) {
      rec[c * FIELDS + F_IMAGE] = (u64)(A.image_base + n);
      rec[c * FIELDS + F_CLASS] = (u64)(c + 1);
    }
}

// 1 <= h, w <= 4096, 2 <= num_classes <= 32, n < 65536, n (num_classes - 1) h w < 2^31
inline bool edt_supported(int64_t n, int64_t h, int64_t w, int32_t num_classes) {
  if (n <= 0 || h <= 0 || w <= 0 || n >= 65536 || h > MAX_SIDE || w > MAX_SIDE) return false;
  if (num_classes < 2 || num_classes > MAX_CLASSES) return false;
  return n * (num_classes - 1) * h * w < (1LL << 31);  // below 2^16 * 2^5 * 2^24: no overflow
}

}  // namespace

extern "C" size_t unet_boundary_distance_sq_workspace(int64_t n, int64_t h, int64_t w, int32_t num_classes) {
  if (!edt_supported(n, h, w, num_classes)) return 0;
  return up16((size_t)(n * (num_classes - 1)) * sizeof(int));
}

extern "C" int32_t unet_boundary_distance_sq(const uint8_t* classes, int64_t n, int64_t h, int64_t w, int32_t num_classes,
                                             int32_t* d2_out, void* workspace, size_t workspace_bytes, void* stream) {
  UNET_REQUIRE(classes && d2_out && workspace, UNET_ERR_BAD_ARG, "unet_boundary_distance_sq: null pointer");
  UNET_REQUIRE(n > 0 && h > 0 && w > 0, UNET_ERR_BAD_ARG, "unet_boundary_distance_sq: n=%lld h=%lld w=%lld", (long long)n,
               (long long)h, (long long)w);
  UNET_REQUIRE(edt_supported(n, h, w, num_classes), UNET_ERR_UNSUPPORTED,
               "unet_boundary_distance_sq: n=%lld h=%lld w=%lld num_classes=%d (h, w <= 4096, 2..32 classes, n < 65536, "
               "n (num_classes - 1) h w < 2^31)", (long long)n, (long long)h, (long long)w, (int)num_classes);
  const size_t need = unet_boundary_distance_sq_workspace(n, h, w, num_classes);
  UNET_REQUIRE(workspace_bytes >= need, UNET_ERR_WORKSPACE, "unet_boundary_distance_sq: workspace too small");
  UNET_REQUIRE(((uintptr_t)workspace & 3) == 0, UNET_ERR_BAD_ARG, "unet_boundary_distance_sq: workspace is not 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int fg = num_classes - 1;
  const double cells = (double)n * fg * h * w;
  UNET_REQUIRE(hipMemsetAsync(workspace, 0, (size_t)(n * fg) * sizeof(int), s) == hipSuccess, UNET_ERR_LAUNCH,
               "unet_boundary_distance_sq: memset failed");
  {
    ColParams A{classes, d2_out, (int*)workspace, (int)h, (int)w, (int)num_classes};
    // the labels once per class group, the planes written, read and written again
    ProfScope prof(UNET_K_OTHER, 0.0, s, "edt_column_pass", (double)n * h * w * cdiv(fg, CG) + cells * 12.0);
    hipLaunchKernelGGL(edt_column_pass, dim3((unsigned)cdiv64(w, COL_THREADS), (unsigned)n, (unsigned)cdiv(fg, CG)),
                       dim3(COL_THREADS), 0, s, A);
    const int32_t rc = unet_check_launch("edt_column_pass");
    if (rc) return rc;
  }
  RowParams B{d2_out, (const int*)workspace, (int)h, (int)w, fg};
  ProfScope prof(UNET_K_OTHER, 0.0, s, "edt_row_pass", cells * 8.0);
  hipLaunchKernelGGL(edt_row_pass, dim3((unsigned)h, (unsigned)fg, (unsigned)n), dim3(ROW_THREADS), 0, s, B);
  return unet_check_launch("edt_row_pass");
}

extern "C" int32_t unet_boundary_stats(const uint8_t* truth, const uint8_t* pred, const int32_t* d2_truth,
                                       const int32_t* d2_pred, int64_t n, int64_t h, int64_t w, int32_t num_classes,
                                       const int32_t* tol_sq, int32_t k, int32_t band_sq, int32_t image_base,
                                       int64_t* records, int64_t* hist, void* stream) {
  UNET_REQUIRE(truth && pred && d2_truth && d2_pred && records && hist && (tol_sq || k == 0), UNET_ERR_BAD_ARG,
               "unet_boundary_stats: null pointer");
  UNET_REQUIRE(n > 0 && h > 0 && w > 0 && image_base >= 0, UNET_ERR_BAD_ARG,
               "unet_boundary_stats: n=%lld h=%lld w=%lld image_base=%d", (long long)n, (long long)h, (long long)w,
               (int)image_base);
  UNET_REQUIRE(k >= 0 && k <= MAX_TOL && band_sq >= 0 && band_sq < NONE, UNET_ERR_BAD_ARG,
               "unet_boundary_stats: k=%d tolerances (at most 4), band_sq=%d (0 .. 2^30 - 1)", (int)k, (int)band_sq);
  for (int i = 0; i < k; ++i)
    UNET_REQUIRE(tol_sq[i] >= 0 && tol_sq[i] < NONE, UNET_ERR_BAD_ARG, "unet_boundary_stats: tol_sq[%d]=%d (0 .. 2^30 - 1)",
                 i, (int)tol_sq[i]);
  UNET_REQUIRE(edt_supported(n, h, w, num_classes) && (int64_t)image_base + n <= (1LL << 31) - 1, UNET_ERR_UNSUPPORTED,
               "unet_boundary_stats: n=%lld h=%lld w=%lld num_classes=%d image_base=%d (h, w <= 4096, 2..32 classes, "
               "n < 65536, n (num_classes - 1) h w < 2^31, image indices below 2^31)", (long long)n, (long long)h,
               (long long)w, (int)num_classes, (int)image_base);
  hipStream_t s = (hipStream_t)stream;
  StatParams A{truth, pred, d2_truth, d2_pred, (int)num_classes, (int)k, (int)band_sq, (int)image_base, {0, 0, 0, 0},
               (long long)(h * w), (u64*)records, (u64*)hist};
  for (int i = 0; i < k; ++i) A.tol_sq[i] = tol_sq[i];
  // both label maps once; of the distance maps about a plane each (a pixel reads its own class's)
  ProfScope prof(UNET_K_OTHER, 0.0, s, "boundary_stats", (double)n * h * w * 10.0);
  hipLaunchKernelGGL(boundary_stats, dim3((unsigned)cdiv64(h * w, ST_THREADS * ST_ITEMS), (unsigned)n), dim3(ST_THREADS),
                     0, s, A);
  return unet_check_launch("boundary_stats");
}
