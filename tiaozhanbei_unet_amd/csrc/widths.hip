// Channel widths that are not multiples of 64 (DoubleConv / Down / Up / OutConv with any widths).
// A layer of c channels runs as the layer of cp = pad64(c) channels whose extra weight rows / columns and BatchNorm
// parameters are zero: the activation's pad lanes stay exactly 0 through every existing kernel.  This file holds the
// small kernels that cross between the parameter's logical shape and the padded one:
//   - conv weight packs with the segment map of a narrow skip (unet_seg_col, common.h);
//   - pad / unpad of fp32 parameters, buffers and gradients, up to UNET_REMAP_MAX tensors per launch;
//   - the gradient of a narrow block's logical-shape output widened into the padded NHWC operator layout.
#include "common.h"

namespace {

inline int wd_blocks(long long items) { return (int)std::min<long long>(cdiv64(items, 256), 256 * 16); }

template <typename T>
__global__ __launch_bounds__(256) void pack_weight_seg_kernel(const float* __restrict__ w, T* __restrict__ out, int Co,
                                                              int Ci, int rows, int K, int mode, int split,
                                                              long long total, const float* __restrict__ scale) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
    out[i] = ET<T>::from_f(unet_pack_seg_value(w, Co, Ci, rows, K, mode, split, i, scale));
}

struct RemapArgs {
  unet_remap_desc d[UNET_REMAP_MAX];
};

// padded column of logical column j (inverse of unet_seg_col)
__device__ inline int seg_pos(int j, int split) { return (split > 0 && j >= split) ? j - split + (split + 63) / 64 * 64 : j; }

// blockIdx.y = descriptor; grid-stride over the elements of the tensor that is written
__global__ __launch_bounds__(256) void remap_batched_kernel(RemapArgs args) {
  const unet_remap_desc d = args.d[blockIdx.y];
  const int inner = d.inner;
  if (d.op == UNET_REMAP_PAD) {                    // padded [prows][pcols][inner] <- logical, zeros elsewhere
    const long long total = (long long)d.prows * d.pcols * inner;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
      const int e = (int)(i % inner);
      const long long t = i / inner;
      const int q = (int)(t % d.pcols), r = (int)(t / d.pcols);
      const int j = unet_seg_col(q, d.split, d.cols);
      d.dst[i] = (r < d.rows && j >= 0) ? d.src[((long long)r * d.cols + j) * inner + e] : 0.f;
    }
  } else {                                         // logical [rows][cols][inner] <- padded
    const long long total = (long long)d.rows * d.cols * inner;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
      const int e = (int)(i % inner);
      const long long t = i / inner;
      const int j = (int)(t % d.cols), r = (int)(t / d.cols);
      d.dst[i] = d.src[((long long)r * d.pcols + seg_pos(j, d.split)) * inner + e];
    }
  }
}

// dst[n][y][x][cp] (NHWC, compute dtype) = src[n][c][y][x] (any strides, fp32 or bf16) for c < C, 0 in the pad lanes
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void widen_channels_kernel(const TI* __restrict__ src, long long sn, long long sc,
                                                             long long sh, long long sw, int N, int C, int H, int W,
                                                             int Cp, TO* __restrict__ dst) {
  const long long total = (long long)N * H * W * Cp;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % Cp);
    long long t = i / Cp;
    const int x = (int)(t % W);
    t /= W;
    const int y = (int)(t % H);
    const long long n = t / H;
    const float v = c < C ? ET<TI>::to_f(src[n * sn + c * sc + y * sh + x * sw]) : 0.f;
    dst[i] = ET<TO>::from_f(v);
  }
}

// pack_weight_seg_kernel over the 9 * rows * k elements of a packed 3x3 weight; scale (may be NULL): BatchNorm fold
int32_t launch_pack_seg(const char* who, int dtype, const float* w, void* out, int c_out, int c_in, int rows, int k, int mode,
                        int split, const float* scale, void* stream) {
  const long long total = 9LL * rows * k;
  hipStream_t s = (hipStream_t)stream;
  return with_dtype(who, dtype, [&](auto tag) {
    using T = decltype(tag);
    ProfScope prof(UNET_K_PACK, 0.0, s, "pack_weight_seg_kernel");
    hipLaunchKernelGGL(pack_weight_seg_kernel<T>, dim3(wd_blocks(total)), dim3(256), 0, s, w, (T*)out, c_out, c_in, rows, k,
                       mode, split, total, scale);
    return unet_check_launch("pack_weight_seg_kernel");
  });
}

}  // namespace

extern "C" int32_t unet_pack_weight_seg(const float* w, void* out, int32_t c_out, int32_t c_in, int32_t rows, int32_t k,
                                        int32_t mode, int32_t split, int32_t dtype, void* stream) {
  UNET_REQUIRE(w && out, UNET_ERR_BAD_ARG, "unet_pack_weight_seg: null pointer");
  UNET_REQUIRE(mode == UNET_PACK_CONV_FWD || mode == UNET_PACK_CONV_DGRAD, UNET_ERR_BAD_ARG,
               "unet_pack_weight_seg: mode %d (3x3 conv weights only)", mode);
  UNET_REQUIRE(c_out > 0 && c_in > 0 && split >= 0 && split < c_in, UNET_ERR_BAD_ARG, "unet_pack_weight_seg: bad dims");
  const int need_ci = split > 0 ? (split + 63) / 64 * 64 + (c_in - split) : c_in;
  const int gemm_rows = mode == UNET_PACK_CONV_FWD ? c_out : need_ci, gemm_k = mode == UNET_PACK_CONV_FWD ? need_ci : c_out;
  UNET_REQUIRE(rows >= gemm_rows && k >= gemm_k, UNET_ERR_BAD_ARG, "unet_pack_weight_seg: padded dims too small");
  return launch_pack_seg("unet_pack_weight_seg", dtype, w, out, c_out, c_in, rows, k, mode, split, nullptr, stream);
}

extern "C" int32_t unet_pack_conv_weight_folded_seg(const float* w, const float* scale, void* out, int32_t c_out,
                                                    int32_t c_in, int32_t rows, int32_t k, int32_t split, int32_t dtype,
                                                    void* stream) {
  UNET_REQUIRE(w && scale && out, UNET_ERR_BAD_ARG, "unet_pack_conv_weight_folded_seg: null pointer");
  UNET_REQUIRE(c_out > 0 && c_in > 0 && split >= 0 && split < c_in, UNET_ERR_BAD_ARG,
               "unet_pack_conv_weight_folded_seg: bad dims");
  const int need_ci = split > 0 ? (split + 63) / 64 * 64 + (c_in - split) : c_in;
  UNET_REQUIRE(rows >= c_out && k >= need_ci, UNET_ERR_BAD_ARG, "unet_pack_conv_weight_folded_seg: padded dims too small");
  return launch_pack_seg("unet_pack_conv_weight_folded_seg", dtype, w, out, c_out, c_in, rows, k, UNET_PACK_CONV_FWD, split,
                         scale, stream);
}

extern "C" int32_t unet_remap_batched(const unet_remap_desc* descs, int32_t n, void* stream) {
  UNET_REQUIRE(descs && n > 0, UNET_ERR_BAD_ARG, "unet_remap_batched: bad argument");
  long long most = 0;
  for (int i = 0; i < n; ++i) {
    const unet_remap_desc& d = descs[i];
    UNET_REQUIRE(d.src && d.dst, UNET_ERR_BAD_ARG, "unet_remap_batched: descriptor %d: null pointer", i);
    UNET_REQUIRE(d.op == UNET_REMAP_PAD || d.op == UNET_REMAP_UNPAD, UNET_ERR_BAD_ARG, "unet_remap_batched: op %d", d.op);
    UNET_REQUIRE(d.rows > 0 && d.cols > 0 && d.inner > 0 && d.split >= 0 && d.split < d.cols && d.prows >= d.rows,
                 UNET_ERR_BAD_ARG, "unet_remap_batched: descriptor %d: bad dims", i);
    const int need = d.split > 0 ? (d.split + 63) / 64 * 64 + (d.cols - d.split) : d.cols;
    UNET_REQUIRE(d.pcols >= need, UNET_ERR_BAD_ARG, "unet_remap_batched: descriptor %d: %d padded columns < %d", i,
                 d.pcols, need);
    const long long items = d.op == UNET_REMAP_PAD ? (long long)d.prows * d.pcols * d.inner
                                                    : (long long)d.rows * d.cols * d.inner;
    most = std::max(most, items);
  }
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(UNET_K_PACK, 0.0, s, "remap_batched_kernel");
  for (int first = 0; first < n; first += UNET_REMAP_MAX) {
    const int m = std::min(n - first, (int)UNET_REMAP_MAX);
    RemapArgs args{};
    for (int i = 0; i < m; ++i) args.d[i] = descs[first + i];
    hipLaunchKernelGGL(remap_batched_kernel, dim3(wd_blocks(most), m), dim3(256), 0, s, args);
  }
  return unet_check_launch("remap_batched_kernel");
}

extern "C" int32_t unet_widen_channels(const void* src, int32_t src_dtype, const int64_t* strides, int32_t n, int32_t c,
                                       int32_t h, int32_t w, void* dst, int32_t c_pad, int32_t dtype, void* stream) {
  UNET_REQUIRE(src && strides && dst, UNET_ERR_BAD_ARG, "unet_widen_channels: null pointer");
  UNET_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0 && c_pad >= c, UNET_ERR_BAD_ARG, "unet_widen_channels: bad dims");
  UNET_REQUIRE(dtype_known(src_dtype), UNET_ERR_BAD_ARG, "unet_widen_channels: src_dtype %d", src_dtype);
  UNET_REQUIRE(dtype_known(dtype), UNET_ERR_BAD_ARG, "unet_widen_channels: dtype %d", dtype);
  const long long total = (long long)n * h * w * c_pad;
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(UNET_K_PACK, 0.0, s, "widen_channels_kernel");
  const dim3 g(wd_blocks(total)), b(256);
  const long long sn = strides[0], sc = strides[1], sh = strides[2], sw = strides[3];
  if (src_dtype == UNET_F32 && dtype == UNET_F32)
    hipLaunchKernelGGL((widen_channels_kernel<float, float>), g, b, 0, s, (const float*)src, sn, sc, sh, sw, n, c, h, w,
                       c_pad, (float*)dst);
  else if (src_dtype == UNET_F32)
    hipLaunchKernelGGL((widen_channels_kernel<float, bf16_t>), g, b, 0, s, (const float*)src, sn, sc, sh, sw, n, c, h, w,
                       c_pad, (bf16_t*)dst);
  else if (dtype == UNET_F32)
    hipLaunchKernelGGL((widen_channels_kernel<bf16_t, float>), g, b, 0, s, (const bf16_t*)src, sn, sc, sh, sw, n, c, h, w,
                       c_pad, (float*)dst);
  else
    hipLaunchKernelGGL((widen_channels_kernel<bf16_t, bf16_t>), g, b, 0, s, (const bf16_t*)src, sn, sc, sh, sw, n, c, h, w,
                       c_pad, (bf16_t*)dst);
  return unet_check_launch("widen_channels_kernel");
}
