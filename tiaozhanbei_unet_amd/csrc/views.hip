// View ensembling (predict_views, eval_views; no reference counterpart: the reference asks its model once per image): the
// logits of V views of one image -- the image resized by a factor, possibly mirrored -- are brought back onto one frame
// of h x w and reduced to one logit map, one label map, one confidence map and a per-pixel count of agreeing views.
//   view_merge    per frame pixel (y, x), over the views in ascending order:
//                   along an axis of N frame and M view samples the tap of output index i is, in integers,
//                     p = floor(((2 i + 1) M 2^15) / N) - 2^15, clamped to [0, (M - 1) 2^16]   ((i + 1/2) M / N - 1/2 in 16.16)
//                     i0 = p >> 16, f = p & 0xFFFF, i1 = min(i0 + 1, M - 1)               (M == N: i0 = i, f = 0)
//                   a flipped axis reads M - 1 - i0 and M - 1 - i1 (the view's logits are those of the mirrored image);
//                     top = ((float)(65536 - fx) a00 + (float)fx a01) 2^-16, bot likewise from a10 and a11,
//                     val = ((float)(65536 - fy) top + (float)fy bot) 2^-16
//                   every product and every sum rounded once (this file is built with -ffp-contract=off); a view of the
//                   frame's own size on both axes is not interpolated: its logits are taken unchanged.
//                   acc_c starts as the first view's value and adds the others; merged_c = acc_c / (float)V.
//                 labels / conf follow from the merged logits by segpixel.h's argmax_conf (first maximum; 1 / sum_j
//                 expf(z_j - max z), j in class order), as in segvis.hip and tiles.hip; agreement counts the views whose
//                 own first maximum is the merged label.
// The gather form: a lane owns output pixels and walks the views; no atomics, no LDS, the outputs are a function of the
// inputs alone.  The view descriptors (at most 16) travel in the kernel arguments and are only indexed by the uniform view
// counter.  A block works on a segment of ONE row, so the y taps and y weights are wave-uniform.  The floor above is two
// 32-bit divisions: t = (2 i + 1) M < 2^29 = q N + r, then floor(t 2^15 / N) = q 2^15 + floor(r 2^15 / N) with r 2^15 < 2^29;
// the 4-pixel lanes divide for their first x and step to the next three by the quotient and remainder of M 2^16 / N, which
// the host supplies.  A lane owns 4 consecutive x (16-byte stores; 16-byte loads of the views of the frame's own size,
// reversed under flip_x) when w is a multiple of 4 and the pointers are aligned, else one pixel.  HBM-bound by its
// bytes: every view logit is read from memory once (the four taps of neighbouring pixels meet in the caches); what it is
// measured to wait for is the number of gathered load instructions, so the two x taps of a row, which are neighbours
// (or one sample at the clamped edge), come in ONE 8-byte load of samples xl, xl + 1 with xl = min(x0, x1, wv - 2), and
// the row bases are scalars with 32-bit lane offsets: 107 -> 78 us on the six-view Gear frame (profiles/view_merge.txt).
#include "segpixel.h"

namespace {

using namespace segpx;                                 // MAXC, aligned, argmax_conf (segpixel.h)
constexpr int MAX_VIEWS = 16;
constexpr int MAX_SIDE = 16384;
constexpr int VM_THREADS = 256;
constexpr int VM_MAX_BLOCKS = 4096;
constexpr float Q16 = 1.0f / 65536.0f;

struct ViewArg {
  const float* z;                                      // [c][hv][wv]
  int hv, wv, flip_x, flip_y;
  unsigned step_q, step_r;                             // (wv << 16) / w and its remainder: the tap numerator's step per x
};

struct MergeArgs {
  ViewArg v[MAX_VIEWS];
  int nv, c, h, w;
  int segs;                                            // blocks' segments per row: cdiv(units per row, blockDim.x)
  long long items;                                     // row segments of the launch
  float* merged; unsigned char* labels; float* conf; unsigned char* agreement;
};

// Q = floor(((2 i + 1) M 2^15) / N), R its remainder; 0 <= i < N, 1 <= M, N <= 16384: t < 2^29, Q < 2^30 + 2^15
__device__ __forceinline__ void tap_divide(int i, int M, int N, unsigned& Q, unsigned& R) {
  const unsigned n = (unsigned)N, t = (unsigned)(2 * i + 1) * (unsigned)M;
  const unsigned q = t / n, s = (t - q * n) << 15;
  const unsigned q2 = s / n;
  Q = (q << 15) + q2;
  R = s - q2 * n;
}

// the clamped tap of Q; with `flip` the mirrored samples
__device__ __forceinline__ void tap_of(unsigned Q, int M, int flip, int& i0, int& i1, int& f) {
  const int p = max(0, min((int)Q - 32768, (M - 1) << 16));
  i0 = p >> 16;
  f = p & 0xFFFF;
  i1 = min(i0 + 1, M - 1);
  if (flip) { i0 = M - 1 - i0; i1 = M - 1 - i1; }
}

// base[i] through a 32-bit byte offset (i < 16384): a scalar base plus a lane offset, no 64-bit address per lane
__device__ __forceinline__ float at_byte(const float* base, int i) {
  return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + ((unsigned)i << 2));
}

// base[i], base[i + 1] in one 8-byte load that is only 4-byte aligned
typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));
__device__ __forceinline__ f32x2u pair_at_byte(const float* base, int i) {
  return *reinterpret_cast<const f32x2u*>(reinterpret_cast<const char*>(base) + ((unsigned)i << 2));
}

__device__ __forceinline__ float lerp16(int f, float a, float b) {
  const float pa = (float)(65536 - f) * a, pb = (float)f * b;
  const float s = pa + pb;
  return s * Q16;
}

// item = frame row y x segment; PX pixels per lane; CM = 4 or 8 class slots in registers
template <int PX, int CM>
__global__ __launch_bounds__(VM_THREADS) void view_merge(const MergeArgs A) {
  const long long frame_plane = (long long)A.h * A.w;
  for (long long item = blockIdx.x; item < A.items; item += gridDim.x) {
    const int y = (int)(item / A.segs);
    const int x = ((int)(item % A.segs) * (int)blockDim.x + (int)threadIdx.x) * PX;
    if (x >= A.w) continue;
    float acc[CM][PX];
    unsigned long long votes[PX];                      // 3 bits per view: its own first maximum
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      votes[k] = 0ull;
#pragma unroll
      for (int c = 0; c < CM; ++c) acc[c][k] = 0.f;
    }
    for (int v = 0; v < A.nv; ++v) {
      const ViewArg& D = A.v[v];
      const long long view_plane = (long long)D.hv * D.wv;
      const bool same = D.hv == A.h && D.wv == A.w;    // uniform
      int y0, y1, fy;
      {
        unsigned Q, R;
        tap_divide(y, D.hv, A.h, Q, R);
        tap_of(Q, D.hv, D.flip_y, y0, y1, fy);
        y0 = __builtin_amdgcn_readfirstlane(y0);       // the same in every lane: scalar row bases below
        y1 = __builtin_amdgcn_readfirstlane(y1);
        fy = __builtin_amdgcn_readfirstlane(fy);
      }
      int x0[PX], x1[PX], fx[PX];
      if (!same) {
        unsigned Q, R;
        tap_divide(x, D.wv, A.w, Q, R);
#pragma unroll
        for (int k = 0; k < PX; ++k) {
          tap_of(Q, D.wv, D.flip_x, x0[k], x1[k], fx[k]);
          Q += D.step_q;
          R += D.step_r;
          if (R >= (unsigned)A.w) { Q += 1u; R -= (unsigned)A.w; }
        }
      } else {
#pragma unroll
        for (int k = 0; k < PX; ++k) { x0[k] = x1[k] = 0; fx[k] = 0; }
      }
      const float* r0 = D.z + (long long)y0 * D.wv;
      const float* r1 = D.z + (long long)y1 * D.wv;
      float best[PX];                                  // the view's own first maximum
      int arg[PX];
#pragma unroll
      for (int k = 0; k < PX; ++k) { best[k] = 0.f; arg[k] = 0; }
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        if (c < A.c) {
          float val[PX];
          if (same) {                                  // y0 = y or h - 1 - y, no fraction: a copy
            if constexpr (PX == 4) {
              const int xs = D.flip_x ? A.w - 4 - x : x;
              const f32x4 t4 = *reinterpret_cast<const f32x4*>(r0 + c * view_plane + xs);
              if (D.flip_x) { val[0] = t4[3]; val[1] = t4[2]; val[2] = t4[1]; val[3] = t4[0]; }
              else { val[0] = t4[0]; val[1] = t4[1]; val[2] = t4[2]; val[3] = t4[3]; }
            } else {
              val[0] = r0[c * view_plane + (D.flip_x ? A.w - 1 - x : x)];
            }
          } else {                                     // uniform row bases, unsigned lane offsets; all taps in flight, then the sums
            const float* p0 = r0 + c * view_plane;
            const float* p1 = r1 + c * view_plane;
            float a00[PX], a01[PX], a10[PX], a11[PX];
            if (D.wv >= 2) {                           // uniform: both x taps lie in the pair at xl, xl + 1 <= wv - 1
#pragma unroll
              for (int k = 0; k < PX; ++k) {
                const int xl = min(min(x0[k], x1[k]), D.wv - 2);
                const f32x2u t = pair_at_byte(p0, xl), b = pair_at_byte(p1, xl);
                a00[k] = x0[k] == xl ? t[0] : t[1]; a01[k] = x1[k] == xl ? t[0] : t[1];
                a10[k] = x0[k] == xl ? b[0] : b[1]; a11[k] = x1[k] == xl ? b[0] : b[1];
              }
            } else {
#pragma unroll
              for (int k = 0; k < PX; ++k) {
                a00[k] = at_byte(p0, x0[k]); a01[k] = at_byte(p0, x1[k]);
                a10[k] = at_byte(p1, x0[k]); a11[k] = at_byte(p1, x1[k]);
              }
            }
#pragma unroll
            for (int k = 0; k < PX; ++k)
              val[k] = lerp16(fy, lerp16(fx[k], a00[k], a01[k]), lerp16(fx[k], a10[k], a11[k]));
          }
#pragma unroll
          for (int k = 0; k < PX; ++k) {
            if (c == 0 || val[k] > best[k]) { best[k] = val[k]; arg[k] = c; }
            acc[c][k] = v == 0 ? val[k] : acc[c][k] + val[k];
          }
        }
      }
#pragma unroll
      for (int k = 0; k < PX; ++k) votes[k] |= (unsigned long long)arg[k] << (3 * v);
    }
    const float nvf = (float)A.nv;
    int label[PX], agree[PX];
    float cf[PX];
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      float z[CM];
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        z[c] = c < A.c ? acc[c][k] / nvf : 0.f;
        acc[c][k] = z[c];
      }
      label[k] = argmax_conf(z, A.c, cf[k]);
      int n = 0;
      for (int v = 0; v < A.nv; ++v) n += (int)((votes[k] >> (3 * v)) & 7ull) == label[k];
      agree[k] = n;
    }
    const long long o = (long long)y * A.w + x;
    if constexpr (PX == 4) {
      if (A.labels)
        *reinterpret_cast<unsigned int*>(A.labels + o) =
            (unsigned)label[0] | ((unsigned)label[1] << 8) | ((unsigned)label[2] << 16) | ((unsigned)label[3] << 24);
      if (A.agreement)
        *reinterpret_cast<unsigned int*>(A.agreement + o) =
            (unsigned)agree[0] | ((unsigned)agree[1] << 8) | ((unsigned)agree[2] << 16) | ((unsigned)agree[3] << 24);
      if (A.conf) {
        const f32x4 t4 = {cf[0], cf[1], cf[2], cf[3]};
        *reinterpret_cast<f32x4*>(A.conf + o) = t4;
      }
      if (A.merged) {
#pragma unroll
        for (int c = 0; c < CM; ++c)
          if (c < A.c) {
            const f32x4 t4 = {acc[c][0], acc[c][1], acc[c][2], acc[c][3]};
            *reinterpret_cast<f32x4*>(A.merged + c * frame_plane + o) = t4;
          }
      }
    } else {
      if (A.labels) A.labels[o] = (unsigned char)label[0];
      if (A.agreement) A.agreement[o] = (unsigned char)agree[0];
      if (A.conf) A.conf[o] = cf[0];
      if (A.merged) {
#pragma unroll
        for (int c = 0; c < CM; ++c)
          if (c < A.c) A.merged[c * frame_plane + o] = acc[c][0];
      }
    }
  }
}

inline bool side_ok(int v) { return v >= 1 && v <= MAX_SIDE; }

}  // namespace

extern "C" int32_t unet_view_merge(const unet_merge_view* views, int32_t n_views, int32_t c, int32_t h, int32_t w,
                                   float* merged, uint8_t* labels, float* conf, uint8_t* agreement, void* stream) {
  const char* who = "unet_view_merge";
  UNET_REQUIRE(n_views >= 1 && n_views <= MAX_VIEWS, UNET_ERR_UNSUPPORTED, "%s: %d views (1..%d)", who, n_views, MAX_VIEWS);
  UNET_REQUIRE(c >= 2 && c <= MAXC, UNET_ERR_UNSUPPORTED, "%s: c=%d (2..8 classes)", who, c);
  UNET_REQUIRE(side_ok(h) && side_ok(w), UNET_ERR_UNSUPPORTED, "%s: a frame of %d x %d (sides 1..%d)", who, h, w, MAX_SIDE);
  UNET_REQUIRE(views != nullptr, UNET_ERR_UNSUPPORTED, "%s: null view array", who);
  UNET_REQUIRE(merged || labels || conf || agreement, UNET_ERR_UNSUPPORTED, "%s: every output is null", who);
  MergeArgs A{};
  bool vec = w % 4 == 0 && (!merged || aligned(merged, 16)) && (!conf || aligned(conf, 16)) &&
             (!labels || aligned(labels, 4)) && (!agreement || aligned(agreement, 4));
  double bytes = (double)h * w * ((merged ? 4.0 * c : 0.0) + (labels ? 1.0 : 0.0) + (conf ? 4.0 : 0.0) + (agreement ? 1.0 : 0.0));
  for (int v = 0; v < n_views; ++v) {
    const unet_merge_view& s = views[v];
    UNET_REQUIRE(s.logits != nullptr, UNET_ERR_UNSUPPORTED, "%s: view %d has a null pointer", who, v);
    UNET_REQUIRE(side_ok(s.h) && side_ok(s.w), UNET_ERR_UNSUPPORTED, "%s: view %d of %d x %d (sides 1..%d)", who, v, s.h,
                 s.w, MAX_SIDE);
    UNET_REQUIRE((s.flip_x == 0 || s.flip_x == 1) && (s.flip_y == 0 || s.flip_y == 1), UNET_ERR_UNSUPPORTED,
                 "%s: view %d has flips %d, %d (0 or 1)", who, v, s.flip_x, s.flip_y);
    const unsigned long long step = (unsigned long long)s.w << 16;
    A.v[v] = ViewArg{s.logits, s.h, s.w, s.flip_x, s.flip_y, (unsigned)(step / (unsigned)w), (unsigned)(step % (unsigned)w)};
    if (s.h == h && s.w == w) vec = vec && aligned(s.logits, 16);       // the 16-byte loads of the views not interpolated
    bytes += 4.0 * c * s.h * s.w;
  }
  A.nv = n_views; A.c = c; A.h = h; A.w = w;
  A.merged = merged; A.labels = labels; A.conf = conf; A.agreement = agreement;
  // block = the row's units rounded up to whole waves, at most VM_THREADS; grid-stride over the row segments
  const int units = cdiv(w, vec ? 4 : 1);
  unsigned threads = (unsigned)(cdiv(units, WAVE) * WAVE);
  if (threads > VM_THREADS) threads = VM_THREADS;
  A.segs = cdiv(units, (int)threads);
  A.items = (long long)h * A.segs;
  const unsigned blocks = (unsigned)(A.items < VM_MAX_BLOCKS ? A.items : VM_MAX_BLOCKS);
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(UNET_K_OTHER, 0.0, s, "view_merge", bytes);
  const auto kernel = vec ? (c <= 4 ? view_merge<4, 4> : view_merge<4, MAXC>)
                          : (c <= 4 ? view_merge<1, 4> : view_merge<1, MAXC>);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, s, A);
  return unet_check_launch("view_merge");
}
