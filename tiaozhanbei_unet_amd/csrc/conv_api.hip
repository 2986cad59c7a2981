// The convolution entry points of the C ABI (include/unet_hip.h): argument checks, the IgemmParams / ConvTParams of a
// launch, and dispatch<>, which picks the kernel family (igemm.hip, conv3.hip, conv3_pdma.hip, conv3_ws.hip,
// convt_ws.hip, convt_gemm.hip) for a layer's shape.  No kernel lives here.
#include "conv_common.h"

namespace {

// The specialised 3x3 kernels address one image plane of every view with 32-bit buffer offsets (descriptor
// num_records and voffset): a plane of 2 GiB or more (e.g. 4096x4096x64 bf16) must take the generic kernel, whose
// addressing is 64-bit.
template <typename T>
inline bool planes_fit_32bit(const IgemmParams& P) {
  auto ok = [](long long h, long long w, long long c) { return h * w * c * (long long)sizeof(T) < 0x7FFFFFFFLL; };
  return ok(P.src[0].H, P.src[0].W, P.src[0].C) && ok(P.src[1].H, P.src[1].W, P.src[1].C) &&
         ok(P.dst[0].H, P.dst[0].W, P.dst[0].C) && ok(P.dst[1].H, P.dst[1].W, P.dst[1].C);
}

template <typename T, int TAPS>
int32_t dispatch(IgemmParams& P, int kclass, hipStream_t s, int* stat_parts = nullptr) {
  if (stat_parts) *stat_parts = 0;
  constexpr int CK4 = 4 * ET<T>::KGC;
  UNET_REQUIRE(P.Cout % 64 == 0, UNET_ERR_UNSUPPORTED, "igemm: c_out %d is not a multiple of 64", P.Cout);
  UNET_REQUIRE(P.Ctot % ET<T>::KGC == 0, UNET_ERR_UNSUPPORTED, "igemm: input channels %d not a multiple of %d",
               P.Ctot, ET<T>::KGC);
  const bool big = (P.Cout % 128 == 0);
  const bool k4 = (P.Ctot % CK4 == 0) && (P.src[1].C == 0 || P.src[0].C % CK4 == 0);
  if (!k4)
    UNET_REQUIRE(P.src[1].C == 0 || P.src[0].C % ET<T>::KGC == 0, UNET_ERR_UNSUPPORTED,
                 "igemm: concat split %d not chunk aligned", P.src[0].C);
  P.nCo = P.Cout / (big ? 128 : 64);
  P.tilesX = cdiv(P.W, TW);
  P.tilesY = cdiv(P.H, TH);
  const bool small = planes_fit_32bit<T>(P);
  if constexpr (TAPS == 9 && sizeof(T) == 2) {
    // 64-channel inputs: weight-stationary streaming kernel
    if (small && P.Ctot == 64 && P.src[1].C == 0) return unet_internal_conv3_ws(P, kclass, s, stat_parts);
    // deep layers (>= 4 input chunks: below that the un-overlapped prologue of the one block per CU costs more
    // than it saves): both operands by LDS-DMA, 512-thread blocks
    const bool dma_ok = small && k4 && P.Ctot >= 128 && P.H % 16 == 0 && P.W % 16 == 0;
    if (dma_ok) return unet_internal_conv3_pdma(P, kclass, s, stat_parts);
  }
  if constexpr (TAPS == 9) {
    if (small && P.Ctot >= 2 * CK4) return unet_internal_conv3<T>(P, big, k4, kclass, s, stat_parts);
  }
  return unet_internal_igemm<T, TAPS>(P, big, k4, kclass, s);
}

template <int TAPS>
int32_t dispatch_dtype(const char* who, int dtype, IgemmParams& P, int kclass, hipStream_t s, int* stat_parts = nullptr) {
  return with_dtype(who, dtype, [&](auto tag) { return dispatch<decltype(tag), TAPS>(P, kclass, s, stat_parts); });
}

inline DView in_view(const unet_view& v) { return DView{(const char*)v.ptr, v.c, v.h, v.w, v.off_y, v.off_x}; }
inline DViewW out_view(const unet_view& v) { return DViewW{(char*)v.ptr, v.c, v.h, v.w, v.off_y, v.off_x}; }
inline DView in_view_or_none(const unet_view& v) { return v.ptr ? in_view(v) : DView{nullptr, 0, 0, 0, 0, 0}; }
inline DViewW out_view_or_none(const unet_view& v) { return v.ptr ? out_view(v) : DViewW{nullptr, 0, 0, 0, 0, 0}; }
inline DViewW dense_out(void* p, int c, int h, int w) { return DViewW{(char*)p, c, h, w, 0, 0}; }

// What every 3x3 launch shares; the caller adds what is its own (bias / relu, stats, bn_*, accumulate).
inline IgemmParams conv3_params(int n, int h, int w, DView src0, DView src1, const void* w_packed, int c_out, DViewW dst0,
                                DViewW dst1, int dst_split) {
  IgemmParams P{};
  P.src[0] = src0; P.src[1] = src1;
  P.dst[0] = dst0; P.dst[1] = dst1;
  P.N = n; P.H = h; P.W = w;
  P.Ctot = P.src[0].C + P.src[1].C;
  P.Cout = c_out;
  P.wK = P.Ctot;
  P.w = (const char*)w_packed;
  P.dst_split = dst_split;
  P.imul = 1; P.gtaps = 1; P.omul = 1; P.nZ = 1;
  return P;
}

}  // namespace

extern "C" int32_t unet_conv3x3(int32_t dtype, int32_t n, int32_t h, int32_t w, const unet_view src[2],
                                const void* w_packed, int32_t c_out, const unet_view dst[2],
                                int32_t dst_split, int32_t accumulate, int32_t kclass, void* stream) {
  UNET_REQUIRE(src && dst && w_packed && src[0].ptr && dst[0].ptr, UNET_ERR_BAD_ARG, "unet_conv3x3: null pointer");
  UNET_REQUIRE(n > 0 && h > 0 && w > 0 && c_out > 0, UNET_ERR_BAD_ARG, "unet_conv3x3: bad dims");
  UNET_REQUIRE(dst_split == c_out || dst[1].ptr, UNET_ERR_BAD_ARG, "unet_conv3x3: dst[1] missing");
  UNET_REQUIRE(dst_split % 64 == 0 && dst_split > 0 && dst_split <= c_out, UNET_ERR_UNSUPPORTED,
               "unet_conv3x3: dst_split %d", dst_split);
  IgemmParams P = conv3_params(n, h, w, in_view(src[0]), in_view_or_none(src[1]), w_packed, c_out, out_view(dst[0]),
                               out_view_or_none(dst[1]), dst_split);
  P.accumulate = accumulate;
  if (kclass < 0 || kclass >= UNET_K_COUNT) kclass = UNET_K_CONV_FWD;
  return dispatch_dtype<9>("unet_conv3x3", dtype, P, kclass, (hipStream_t)stream);
}

extern "C" int32_t unet_conv3x3_bias_relu(int32_t dtype, int32_t n, int32_t h, int32_t w, const unet_view src[2],
                                          const void* w_packed, int32_t c_out, void* y, const float* bias,
                                          int32_t relu, void* stream) {
  UNET_REQUIRE(src && w_packed && src[0].ptr && y && bias, UNET_ERR_BAD_ARG, "unet_conv3x3_bias_relu: null pointer");
  UNET_REQUIRE(n > 0 && h > 0 && w > 0 && c_out > 0, UNET_ERR_BAD_ARG, "unet_conv3x3_bias_relu: bad dims");
  IgemmParams P = conv3_params(n, h, w, in_view(src[0]), in_view_or_none(src[1]), w_packed, c_out, dense_out(y, c_out, h, w),
                               DViewW{}, c_out);
  P.bias = bias;
  P.relu = relu;
  return dispatch_dtype<9>("unet_conv3x3_bias_relu", dtype, P, UNET_K_CONV_FWD, (hipStream_t)stream);
}

extern "C" size_t unet_conv3x3_stats_max_parts(int32_t n, int32_t h, int32_t w) {
  const size_t tiles = (size_t)n * cdiv(h, TH) * cdiv(w, TW);
  return tiles > 1024 ? tiles : 1024;
}

extern "C" int32_t unet_conv3x3_stats(int32_t dtype, int32_t n, int32_t h, int32_t w, const unet_view src[2],
                                      const void* w_packed, int32_t c_out, void* y, float* partial,
                                      int32_t* n_parts, void* stream) {
  UNET_REQUIRE(src && w_packed && src[0].ptr && y && partial && n_parts, UNET_ERR_BAD_ARG,
               "unet_conv3x3_stats: null pointer");
  UNET_REQUIRE(n > 0 && h > 0 && w > 0 && c_out > 0, UNET_ERR_BAD_ARG, "unet_conv3x3_stats: bad dims");
  IgemmParams P = conv3_params(n, h, w, in_view(src[0]), in_view_or_none(src[1]), w_packed, c_out, dense_out(y, c_out, h, w),
                               DViewW{}, c_out);
  P.stats = partial;
  hipStream_t s = (hipStream_t)stream;
  int parts = 0;
  int32_t rc = dispatch_dtype<9>("unet_conv3x3_stats", dtype, P, UNET_K_CONV_FWD, s, &parts);
  if (rc) return rc;
  if (parts == 0)   // this kernel variant has no fused statistics: one streaming pass over y instead
    rc = unet_internal_bn_partials(dtype, y, (int64_t)n * h * w, c_out, partial, &parts, s);
  *n_parts = parts;
  return rc;
}

// ---- data gradient of a 3x3 convolution fused with the ReLU mask and the BatchNorm-backward sums of the layer that
// produced the convolution's input (the internal activation of DoubleConv, src/model.py:14-19)
namespace {
inline bool dgrad_bnrelu_pdma_ok(int dtype, int n, int h, int w, int c_in_gemm, int c_out_gemm) {
  (void)n;
  return dtype == UNET_BF16 && c_in_gemm >= 128 && c_in_gemm % 64 == 0 && c_out_gemm % 64 == 0 && h % 16 == 0 &&
         w % 16 == 0 && (long long)h * w * c_out_gemm * 2 < 0x7FFFFFFFLL && (long long)h * w * c_in_gemm * 2 < 0x7FFFFFFFLL;
}
// 64 -> 64 (the full-resolution level): the weight-stationary streaming kernel, any frame size
inline bool dgrad_bnrelu_ws_ok(int dtype, int n, int h, int w, int c_in_gemm, int c_out_gemm) {
  (void)n;
  return dtype == UNET_BF16 && c_in_gemm == 64 && c_out_gemm == 64 && (long long)h * w * 64 * 2 < 0x7FFFFFFFLL;
}
}  // namespace

extern "C" int32_t unet_conv3x3_dgrad_bnrelu_supported(int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c_dy,
                                                       int32_t c_dx) {
  return (dgrad_bnrelu_pdma_ok(dtype, n, h, w, c_dy, c_dx) || dgrad_bnrelu_ws_ok(dtype, n, h, w, c_dy, c_dx)) ? 1 : 0;
}

extern "C" int32_t unet_conv3x3_dgrad_bnrelu(int32_t dtype, int32_t n, int32_t h, int32_t w, const void* dy, int32_t c_dy,
                                             const void* w_packed, int32_t c_dx, const void* y_prev,
                                             const float* bn_scale, const float* bn_shift, const float* bn_mean,
                                             void* dz, float* partial, int32_t* n_parts, void* stream) {
  UNET_REQUIRE(dy && w_packed && y_prev && bn_scale && bn_shift && bn_mean && dz && partial && n_parts, UNET_ERR_BAD_ARG,
               "unet_conv3x3_dgrad_bnrelu: null pointer");
  UNET_REQUIRE(n > 0 && h > 0 && w > 0, UNET_ERR_BAD_ARG, "unet_conv3x3_dgrad_bnrelu: bad dims");
  UNET_REQUIRE(dtype_known(dtype), UNET_ERR_BAD_ARG, "unet_conv3x3_dgrad_bnrelu: dtype %d", dtype);
  UNET_REQUIRE(unet_conv3x3_dgrad_bnrelu_supported(dtype, n, h, w, c_dy, c_dx), UNET_ERR_UNSUPPORTED,
               "unet_conv3x3_dgrad_bnrelu: %d -> %d channels at %dx%d (dtype %d) is not covered; use unet_conv3x3 + "
               "unet_bn_relu_bwd", c_dy, c_dx, h, w, dtype);
  IgemmParams P = conv3_params(n, h, w, DView{(const char*)dy, c_dy, h, w, 0, 0}, DView{}, w_packed, c_dx,
                               dense_out(dz, c_dx, h, w), DViewW{}, c_dx);
  P.stats = partial;
  P.bn_y = (const char*)y_prev;
  P.bn_scale = bn_scale; P.bn_shift = bn_shift; P.bn_mean = bn_mean;
  int parts = 0;
  hipStream_t s = (hipStream_t)stream;
  int32_t rc;
  if (dgrad_bnrelu_pdma_ok(dtype, n, h, w, c_dy, c_dx))
    rc = unet_internal_conv3_pdma(P, UNET_K_CONV_DGRAD, s, &parts);
  else
    rc = unet_internal_conv3_ws(P, UNET_K_CONV_DGRAD, s, &parts);
  *n_parts = parts;
  return rc;
}

extern "C" int32_t unet_convt2x2_fwd(int32_t dtype, int32_t n, int32_t h, int32_t w, const void* x,
                                     int32_t c_in, const void* w_packed, const float* bias, void* y,
                                     int32_t c_out, void* stream) {
  UNET_REQUIRE(x && w_packed && y, UNET_ERR_BAD_ARG, "unet_convt2x2_fwd: null pointer");
  UNET_REQUIRE(n > 0 && h > 0 && w > 0, UNET_ERR_BAD_ARG, "unet_convt2x2_fwd: bad dims");
  {
    const long long out_bytes = (long long)n * 4 * h * w * c_out * 2;
    if (dtype == UNET_BF16 && c_in == 2 * c_out && (c_in == 128 || c_in == 256) && out_bytes < 0x7FFFFFFFLL) {
      ConvTParams T{(const char*)x, (char*)y, (const char*)w_packed, bias, n, h, w, c_out, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr};
      return unet_internal_convt_ws(c_in, T, (hipStream_t)stream);
    }
  }
  if (unet_internal_convt_gemm_ok(0, dtype, n, h, w, c_in, c_out))     // deep levels: one LDS-DMA GEMM (convt_gemm.hip)
    return unet_internal_convt_gemm(0, n, h, w, x, w_packed, bias, y, c_in, c_out, (hipStream_t)stream);
  IgemmParams P{};
  P.src[0] = DView{(const char*)x, c_in, h, w, 0, 0};
  P.dst[0] = DViewW{(char*)y, c_out, 2 * h, 2 * w, 0, 0};
  P.N = n; P.H = h; P.W = w;
  // one GEMM with 4*c_out rows (row = z*c_out + co, the packed layout [4][c_out][c_in] read as one matrix):
  // the input tile is staged once for all four sub-positions
  P.Ctot = c_in; P.Cout = 4 * c_out; P.wK = c_in;
  P.w = (const char*)w_packed;
  P.bias = bias;
  P.dst_split = 4 * c_out;
  P.imul = 1; P.gtaps = 1; P.omul = 2; P.nZ = 1; P.zdiv = c_out;
  return dispatch_dtype<1>("unet_convt2x2_fwd", dtype, P, UNET_K_CONVT_FWD, (hipStream_t)stream);
}

extern "C" int32_t unet_convt2x2_dgrad(int32_t dtype, int32_t n, int32_t h, int32_t w, const void* dy,
                                       int32_t c_out, const void* w_packed, void* dx, int32_t c_in,
                                       void* stream) {
  UNET_REQUIRE(dy && w_packed && dx, UNET_ERR_BAD_ARG, "unet_convt2x2_dgrad: null pointer");
  UNET_REQUIRE(n > 0 && h > 0 && w > 0, UNET_ERR_BAD_ARG, "unet_convt2x2_dgrad: bad dims");
  {
    const long long in_bytes = (long long)n * 4 * h * w * c_out * 2;
    if (dtype == UNET_BF16 && c_in == 2 * c_out && (c_out == 64 || c_out == 128) && in_bytes < 0x7FFFFFFFLL) {
      ConvTParams T{(const char*)dy, (char*)dx, (const char*)w_packed, nullptr, n, h, w, c_out, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr};
      return unet_internal_convt_dgrad_ws(c_out, T, (hipStream_t)stream);
    }
  }
  if (unet_internal_convt_gemm_ok(1, dtype, n, h, w, c_in, c_out))
    return unet_internal_convt_gemm(1, n, h, w, dy, w_packed, nullptr, dx, c_in, c_out, (hipStream_t)stream);
  IgemmParams P{};
  P.src[0] = DView{(const char*)dy, c_out, 2 * h, 2 * w, 0, 0};
  P.dst[0] = DViewW{(char*)dx, c_in, h, w, 0, 0};
  P.N = n; P.H = h; P.W = w;
  P.Ctot = c_out; P.Cout = c_in; P.wK = 4 * c_out;
  P.w = (const char*)w_packed;
  P.bias = nullptr;
  P.dst_split = c_in;
  P.imul = 2; P.gtaps = 4; P.omul = 1; P.nZ = 1;
  return dispatch_dtype<1>("unet_convt2x2_dgrad", dtype, P, UNET_K_CONVT_DGRAD, (hipStream_t)stream);
}

// ---- data gradient of a transposed convolution fused with the ReLU mask and the BatchNorm-backward sums of the layer that
// produced its input (the DoubleConv in front of an Up block, src/model.py:14-19 -> :51)
extern "C" int32_t unet_convt2x2_dgrad_bnrelu_supported(int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c_in,
                                                        int32_t c_out) {
  const long long in_bytes = (long long)n * 4 * h * w * c_out * 2;
  // (c_out == 128 -- 128 weight registers per lane -- has no room for the running sums: 78 spills; not offered)
  return (dtype == UNET_BF16 && c_in == 2 * c_out && c_out == 64 && in_bytes < 0x7FFFFFFFLL) ? 1 : 0;
}

extern "C" size_t unet_convt2x2_dgrad_bnrelu_max_parts(void) { return 256; }

extern "C" int32_t unet_convt2x2_dgrad_bnrelu(int32_t dtype, int32_t n, int32_t h, int32_t w, const void* dy, int32_t c_out,
                                              const void* w_packed, const void* y_prev, const float* bn_scale,
                                              const float* bn_shift, const float* bn_mean, void* dz, int32_t c_in,
                                              float* partial, int32_t* n_parts, void* stream) {
  UNET_REQUIRE(dy && w_packed && y_prev && bn_scale && bn_shift && bn_mean && dz && partial && n_parts, UNET_ERR_BAD_ARG,
               "unet_convt2x2_dgrad_bnrelu: null pointer");
  UNET_REQUIRE(n > 0 && h > 0 && w > 0, UNET_ERR_BAD_ARG, "unet_convt2x2_dgrad_bnrelu: bad dims");
  UNET_REQUIRE(dtype_known(dtype), UNET_ERR_BAD_ARG, "unet_convt2x2_dgrad_bnrelu: dtype %d", dtype);
  UNET_REQUIRE(unet_convt2x2_dgrad_bnrelu_supported(dtype, n, h, w, c_in, c_out), UNET_ERR_UNSUPPORTED,
               "unet_convt2x2_dgrad_bnrelu: %d <- %d channels at %dx%d (dtype %d) is not covered; use unet_convt2x2_dgrad + "
               "unet_bn_relu_bwd", c_in, c_out, h, w, dtype);
  ConvTParams T{(const char*)dy, (char*)dz, (const char*)w_packed, nullptr, n, h, w, c_out, 0, 0,
                (const char*)y_prev, bn_scale, bn_shift, bn_mean, partial};
  int parts = 0;
  const int32_t rc = unet_internal_convt_dgrad_ws(64, T, (hipStream_t)stream, &parts);
  *n_parts = parts;
  return rc;
}

#ifdef PDMA_STAMPS
// diagnostic build only (not in unet_hip.h; tools/stamps.py binds it itself): the stamp records of every stamped
// kernel (stamps.h) go to p, room for `records` records of eight uint64; nullptr switches the write-out off
StampSink g_stamp_sink = {nullptr, 0};
extern "C" void unet_debug_set_buffer(void* p, int64_t records) { g_stamp_sink = {(unsigned long long*)p, p ? records : 0}; }
#endif
