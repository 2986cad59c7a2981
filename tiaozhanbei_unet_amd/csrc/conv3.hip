// conv3_kernel: the 3x3 specialisation (forward and data gradient).  Same tiling as igemm_kernel (igemm.hip), but
//  * the 9 taps are fully unrolled (tap shift = immediate LDS offset, exact counted vmcnt waits),
//  * weight slabs are prefetched TWO steps ahead into two named register sets (an L2/HBM round trip is
//    longer than one 16-MFMA step),
//  * the next chunk's halo patch is prefetched into registers three taps before it is needed,
//  * all staging addresses are per-thread constants (+ a scalar base per step): no index math in the loop,
//  * halo rows are padded to a multiple of 256 B so the two pixel rows of a 32-lane MFMA operand land on
//    disjoint banks (ds_read_b128 conflict-free; the unpadded layout was 2-way).
#include "conv_common.h"

namespace {

template <typename T, int BN, int KG>
struct Cfg3 {
  static constexpr int HH = TH + 2, HW = TW + 2;
  static constexpr int CHB = KG * 32, PSTR = CHB + 16, PPP = CHB / 16;
  static constexpr int RS = (HW * PSTR + 255) / 256 * 256;   // halo row stride (bytes)
  static constexpr int A_BYTES = HH * RS;
  static constexpr int B_BYTES = BN * PSTR;
  static constexpr int LDS = A_BYTES + 2 * B_BYTES;
  static constexpr int CK = KG * ET<T>::KGC;
  static constexpr int WCO = BN / 64, WPX = 4 / WCO, PXT = NPIX / (32 * WPX);
  static constexpr int NAP = (HH * HW * PPP + 255) / 256;
  static constexpr int NBP = (BN * PPP + 255) / 256;
};

template <typename T, int BN, int KG>
__global__ __launch_bounds__(256, 2) void conv3_kernel(const IgemmParams P) {
  using C = Cfg3<T, BN, KG>;
  using E = ET<T>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const sA = smem;
  char* const sB = smem + C::A_BYTES;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wco = wave % C::WCO, wpx = wave / C::WCO;
  const int l31 = lane & 31, hh = lane >> 5;

  int logical;
  {
    const int total = gridDim.x, b = blockIdx.x;
    const int xcd = b & 7, slot = b >> 3, q = total >> 3, r = total & 7;
    logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
  }
  const int cot = logical % P.nCo;
  int t = logical / P.nCo;
  const int txi = t % P.tilesX;  t /= P.tilesX;
  const int tyi = t % P.tilesY;
  const int n = t / P.tilesY;
  const int ty0 = tyi * TH, tx0 = txi * TW;
  const int co0 = cot * BN;

  f32x16 acc[2][C::PXT];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < C::PXT; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  int aoff[2], boff[C::PXT];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) aoff[ct] = (wco * 64 + ct * 32 + l31) * C::PSTR + hh * 16;
#pragma unroll
  for (int pt = 0; pt < C::PXT; ++pt) {
    const int m = wpx * (32 * C::PXT) + pt * 32 + l31;
    boff[pt] = (m >> 4) * C::RS + (m & 15) * C::PSTR + hh * 16;
  }

  // ---- per-thread staging descriptors (constant for the whole block).  Loads are buffer loads: a
  // wave-uniform resource (SGPRs) + per-thread constant voffset + per-step scalar soffset, so the loop
  // carries no address VALU; out-of-image halo pixels use an out-of-range voffset and read as zero.
  constexpr unsigned OOB = 0xFFFFFFF0u;
  constexpr bool A_EXACT = (C::HH * C::HW * C::PPP) % 256 == 0;
  constexpr bool B_EXACT = (BN * C::PPP) % 256 == 0;
  int a_lds[C::NAP];
  unsigned a_g[2][C::NAP];
#pragma unroll
  for (int i = 0; i < C::NAP; ++i) {
    const int id = tid + i * 256;
    a_lds[i] = -1;
    a_g[0][i] = a_g[1][i] = OOB;
    if (id < C::HH * C::HW * C::PPP) {
      const int pix = id / C::PPP, part = id % C::PPP;
      const int hy = pix / C::HW, hx = pix - hy * C::HW;
      a_lds[i] = hy * C::RS + hx * C::PSTR + part * 16;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const DView S = P.src[k];
        const int y = ty0 + hy - 1 - S.oy, x = tx0 + hx - 1 - S.ox;
        if (S.C > 0 && y >= 0 && y < S.H && x >= 0 && x < S.W)
          a_g[k][i] = (unsigned)(((y * S.W + x) * S.C) * E::ES + part * 16);
      }
    }
  }
  int b_lds[C::NBP];
  unsigned b_g[C::NBP];
#pragma unroll
  for (int i = 0; i < C::NBP; ++i) {
    const int id = tid + i * 256;
    const int row = id / C::PPP, part = id % C::PPP;
    const bool ok = B_EXACT || id < BN * C::PPP;
    b_lds[i] = ok ? row * C::PSTR + part * 16 : -1;
    b_g[i] = ok ? (unsigned)(((co0 + row) * P.wK) * E::ES + part * 16) : OOB;
  }

  const int nchunks = P.Ctot / C::CK;
  const unsigned w_tap_stride = (unsigned)P.Cout * P.wK * E::ES;
  const __amdgpu_buffer_rsrc_t w_rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)P.w, (short)0, (int)(9u * w_tap_stride), 0x00020000);
  __amdgpu_buffer_rsrc_t a_rsrc[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const DView S = P.src[k];
    const unsigned img = (unsigned)S.H * S.W * S.C * E::ES;
    a_rsrc[k] = __builtin_amdgcn_make_buffer_rsrc((void*)(S.p + (size_t)n * img), (short)0, (int)img, 0x00020000);
  }

  u32x4 breg[2][C::NBP];
  u32x4 areg[C::NAP];

  auto load_b = [&](u32x4 (&dst)[C::NBP], int chunk, int tap) {
    if (tap >= 9) { tap -= 9; chunk += 1; }
    chunk = chunk < nchunks ? chunk : nchunks - 1;        // past the end: harmless re-load, never consumed
    const unsigned soff = (unsigned)tap * w_tap_stride + (unsigned)chunk * (C::CK * E::ES);
#pragma unroll
    for (int i = 0; i < C::NBP; ++i)
      dst[i] = __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, b_g[i], soff, 0);
  };
  auto store_b = [&](const u32x4 (&src)[C::NBP], int buf) {
#pragma unroll
    for (int i = 0; i < C::NBP; ++i)
      if (B_EXACT || b_lds[i] >= 0) *reinterpret_cast<u32x4*>(sB + buf * C::B_BYTES + b_lds[i]) = src[i];
  };
  auto load_a = [&](int chunk) {
    chunk = chunk < nchunks ? chunk : nchunks - 1;
    const int ch = chunk * C::CK;
    if (ch < P.src[0].C) {
      const unsigned soff = (unsigned)ch * E::ES;
#pragma unroll
      for (int i = 0; i < C::NAP; ++i) areg[i] = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc[0], a_g[0][i], soff, 0);
    } else {
      const unsigned soff = (unsigned)(ch - P.src[0].C) * E::ES;
#pragma unroll
      for (int i = 0; i < C::NAP; ++i) areg[i] = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc[1], a_g[1][i], soff, 0);
    }
  };
  auto store_a = [&]() {
#pragma unroll
    for (int i = 0; i < C::NAP; ++i)
      if (A_EXACT || i + 1 < C::NAP || a_lds[i] >= 0) *reinterpret_cast<u32x4*>(sA + a_lds[i]) = areg[i];
  };

  auto compute = [&](int toff, int bbuf) {
    const char* pa = sB + bbuf * C::B_BYTES;
    const char* pb = sA + toff;
#pragma unroll
    for (int kg = 0; kg < KG; ++kg) {
      if constexpr (sizeof(T) == 2) {
        bf16x8 fa[2], fb[C::PXT];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) fa[ct] = *reinterpret_cast<const bf16x8*>(pa + aoff[ct] + kg * 32);
#pragma unroll
        for (int pt = 0; pt < C::PXT; ++pt) fb[pt] = *reinterpret_cast<const bf16x8*>(pb + boff[pt] + kg * 32);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
          for (int pt = 0; pt < C::PXT; ++pt)
            acc[ct][pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ct], fb[pt], acc[ct][pt], 0, 0, 0);
      } else {
        f32x4 fa[2], fb[C::PXT];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) fa[ct] = *reinterpret_cast<const f32x4*>(pa + aoff[ct] + kg * 32);
#pragma unroll
        for (int pt = 0; pt < C::PXT; ++pt) fb[pt] = *reinterpret_cast<const f32x4*>(pb + boff[pt] + kg * 32);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int pt = 0; pt < C::PXT; ++pt)
              acc[ct][pt] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[ct][j], fb[pt][j], acc[ct][pt], 0, 0, 0);
      }
    }
  };

  // one chunk = 9 fully unrolled tap steps; PAR = parity of its first step (selects register set / LDS slot).
  // Step t:  barrier(t) | park slab t+1 in the other LDS slot (its last readers passed barrier(t)) | issue the
  // loads of slab t+3 into the registers just freed | 16 MFMAs on slab t.  The LDS writes of a slab are a
  // whole step old when the barrier that publishes them arrives, so a barrier only ever waits for skew.
  auto chunk_body = [&](int c, auto par_tag) {
    constexpr int PAR = decltype(par_tag)::value;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int set = (PAR + tap) & 1;              // slot / register set of THIS step's slab
      __syncthreads();
      if (tap + 1 < 9 || c + 1 < nchunks) store_b(breg[set ^ 1], set ^ 1);          // slab t+1
      if (tap + 3 < 9 || c + 1 < nchunks) load_b(breg[set ^ 1], c, tap + 3);        // slab t+3 (uniform branch)
      if (tap == 5 && c + 1 < nchunks) load_a(c + 1);
      compute((tap / 3) * C::RS + (tap % 3) * C::PSTR, set);
    }
    if (c + 1 < nchunks) {
      __syncthreads();        // every wave is done with this chunk's patch
      store_a();
    }
  };

  load_a(0);
  load_b(breg[0], 0, 0);
  load_b(breg[1], 0, 1);
  store_a();
  store_b(breg[0], 0);
  load_b(breg[0], 0, 2);
  int c = 0;
  for (; c + 1 < nchunks; c += 2) {
    chunk_body(c, std::integral_constant<int, 0>{});
    chunk_body(c + 1, std::integral_constant<int, 1>{});
  }
  if (c < nchunks) chunk_body(c, std::integral_constant<int, 0>{});

  // ---- epilogue (identical to igemm_kernel, omul = 1, no bias)
#pragma unroll
  for (int pt = 0; pt < C::PXT; ++pt) {
    const int m = wpx * (32 * C::PXT) + pt * 32 + l31;
    const int fy = ty0 + (m >> 4), fx = tx0 + (m & 15);
    if (fy >= P.H || fx >= P.W) continue;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        int co = co0 + wco * 64 + ct * 32 + 8 * g + 4 * hh;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = acc[ct][pt][4 * g + j];
        if (P.bias) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] += P.bias[co + j];
        }
        if (P.relu) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
        }
        const int accq = (co < P.dst_split) ? (P.accumulate & 1) : (P.accumulate & 2);   // per-view accumulate bit
        const DViewW D = (co < P.dst_split) ? P.dst[0] : P.dst[1];
        if (co >= P.dst_split) co -= P.dst_split;
        const int y = fy - D.oy, x = fx - D.ox;
        if (y < 0 || y >= D.H || x < 0 || x >= D.W) continue;
        T* o = reinterpret_cast<T*>(D.p) + ((size_t)(n * D.H + y) * D.W + x) * D.C + co;
        if constexpr (sizeof(T) == 2) {
          if (accq) {
            bf16x4 old = *reinterpret_cast<const bf16x4*>(o);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] += (float)old[j];
          }
          bf16x4 r;
#pragma unroll
          for (int j = 0; j < 4; ++j) r[j] = (bf16_t)v[j];
          *reinterpret_cast<bf16x4*>(o) = r;
        } else {
          if (accq) {
            f32x4 old = *reinterpret_cast<const f32x4*>(o);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] += old[j];
          }
          *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
        }
      }
    }
  }
}

// ---- conv3m16_kernel: conv3_kernel on v_mfma_f32_16x16x32_bf16 (4x4 tiles of 16x16 per wave).  Same bytes
// and MFMA cycles; the chip sustains a higher clock on this shape (MI355X_MICROARCH, DVFS give-back item 7).
template <typename T, int BN, int KG>
struct Cfg3M {
  static constexpr int HH = TH + 2, HW = TW + 2;
  static constexpr int CHB = KG * 32, PSTR = CHB + 32, PPP = CHB / 16;   // +32 B: conflict-free 16x16x32 fragments
  static constexpr int RS = HW * PSTR;                       // a 16-pixel operand never straddles halo rows
  static constexpr int A_BYTES = HH * RS;
  static constexpr int B_BYTES = BN * PSTR;
  static constexpr int LDS = A_BYTES + 2 * B_BYTES;
  static constexpr int CK = KG * ET<T>::KGC;
  static constexpr int WCO = BN / 64, WPX = 4 / WCO, PXT = NPIX / (32 * WPX);
  static constexpr int NAP = (HH * HW * PPP + 255) / 256;
  static constexpr int NBP = (BN * PPP + 255) / 256;
};

template <typename T, int BN, int KG>
__global__ __launch_bounds__(256, 2) void conv3m16_kernel(const IgemmParams P) {
  using C = Cfg3M<T, BN, KG>;
  using E = ET<T>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const sA = smem;
  char* const sB = smem + C::A_BYTES;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wco = wave % C::WCO, wpx = wave / C::WCO;
  
  int logical;
  {
    const int total = gridDim.x, b = blockIdx.x;
    const int xcd = b & 7, slot = b >> 3, q = total >> 3, r = total & 7;
    logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
  }
  const int cot = logical % P.nCo;
  int t = logical / P.nCo;
  const int txi = t % P.tilesX;  t /= P.tilesX;
  const int tyi = t % P.tilesY;
  const int n = t / P.tilesY;
  const int ty0 = tyi * TH, tx0 = txi * TW;
  const int co0 = cot * BN;

  constexpr int PT16 = 2 * C::PXT;              // 16-pixel operand tiles per wave (each = one tile row)
  const int l15 = lane & 15, kb = lane >> 4;
  f32x4 acc[4][PT16];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < PT16; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[a][b][r] = 0.f;

  int aoff[4], boff[PT16];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) aoff[ct] = (wco * 64 + ct * 16 + l15) * C::PSTR + kb * 16;
#pragma unroll
  for (int pt = 0; pt < PT16; ++pt) boff[pt] = (wpx * PT16 + pt) * C::RS + l15 * C::PSTR + kb * 16;

  // ---- per-thread staging descriptors (constant for the whole block).  Loads are buffer loads: a
  // wave-uniform resource (SGPRs) + per-thread constant voffset + per-step scalar soffset, so the loop
  // carries no address VALU; out-of-image halo pixels use an out-of-range voffset and read as zero.
  constexpr unsigned OOB = 0xFFFFFFF0u;
  constexpr bool A_EXACT = (C::HH * C::HW * C::PPP) % 256 == 0;
  constexpr bool B_EXACT = (BN * C::PPP) % 256 == 0;
  int a_lds[C::NAP];
  unsigned a_g[2][C::NAP];
#pragma unroll
  for (int i = 0; i < C::NAP; ++i) {
    const int id = tid + i * 256;
    a_lds[i] = -1;
    a_g[0][i] = a_g[1][i] = OOB;
    if (id < C::HH * C::HW * C::PPP) {
      const int pix = id / C::PPP, part = id % C::PPP;
      const int hy = pix / C::HW, hx = pix - hy * C::HW;
      a_lds[i] = hy * C::RS + hx * C::PSTR + part * 16;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const DView S = P.src[k];
        const int y = ty0 + hy - 1 - S.oy, x = tx0 + hx - 1 - S.ox;
        if (S.C > 0 && y >= 0 && y < S.H && x >= 0 && x < S.W)
          a_g[k][i] = (unsigned)(((y * S.W + x) * S.C) * E::ES + part * 16);
      }
    }
  }
  int b_lds[C::NBP];
  unsigned b_g[C::NBP];
#pragma unroll
  for (int i = 0; i < C::NBP; ++i) {
    const int id = tid + i * 256;
    const int row = id / C::PPP, part = id % C::PPP;
    const bool ok = B_EXACT || id < BN * C::PPP;
    b_lds[i] = ok ? row * C::PSTR + part * 16 : -1;
    b_g[i] = ok ? (unsigned)(((co0 + row) * P.wK) * E::ES + part * 16) : OOB;
  }

  const int nchunks = P.Ctot / C::CK;
  const unsigned w_tap_stride = (unsigned)P.Cout * P.wK * E::ES;
  const __amdgpu_buffer_rsrc_t w_rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)P.w, (short)0, (int)(9u * w_tap_stride), 0x00020000);
  __amdgpu_buffer_rsrc_t a_rsrc[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const DView S = P.src[k];
    const unsigned img = (unsigned)S.H * S.W * S.C * E::ES;
    a_rsrc[k] = __builtin_amdgcn_make_buffer_rsrc((void*)(S.p + (size_t)n * img), (short)0, (int)img, 0x00020000);
  }

  u32x4 breg[2][C::NBP];
  u32x4 areg[C::NAP];

  auto load_b = [&](u32x4 (&dst)[C::NBP], int chunk, int tap) {
    if (tap >= 9) { tap -= 9; chunk += 1; }
    chunk = chunk < nchunks ? chunk : nchunks - 1;        // past the end: harmless re-load, never consumed
    const unsigned soff = (unsigned)tap * w_tap_stride + (unsigned)chunk * (C::CK * E::ES);
#pragma unroll
    for (int i = 0; i < C::NBP; ++i)
      dst[i] = __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, b_g[i], soff, 0);
  };
  auto store_b = [&](const u32x4 (&src)[C::NBP], int buf) {
#pragma unroll
    for (int i = 0; i < C::NBP; ++i)
      if (B_EXACT || b_lds[i] >= 0) *reinterpret_cast<u32x4*>(sB + buf * C::B_BYTES + b_lds[i]) = src[i];
  };
  auto load_a = [&](int chunk) {
    chunk = chunk < nchunks ? chunk : nchunks - 1;
    const int ch = chunk * C::CK;
    if (ch < P.src[0].C) {
      const unsigned soff = (unsigned)ch * E::ES;
#pragma unroll
      for (int i = 0; i < C::NAP; ++i) areg[i] = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc[0], a_g[0][i], soff, 0);
    } else {
      const unsigned soff = (unsigned)(ch - P.src[0].C) * E::ES;
#pragma unroll
      for (int i = 0; i < C::NAP; ++i) areg[i] = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc[1], a_g[1][i], soff, 0);
    }
  };
  auto store_a = [&]() {
#pragma unroll
    for (int i = 0; i < C::NAP; ++i)
      if (A_EXACT || i + 1 < C::NAP || a_lds[i] >= 0) *reinterpret_cast<u32x4*>(sA + a_lds[i]) = areg[i];
  };

  auto compute = [&](int toff, int bbuf) {
    const char* pa = sB + bbuf * C::B_BYTES;
    const char* pb = sA + toff;
#pragma unroll
    for (int ks = 0; ks < KG / 2; ++ks) {       // k steps of 32 channels
      bf16x8 fa[4], fb[PT16];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) fa[ct] = *reinterpret_cast<const bf16x8*>(pa + aoff[ct] + ks * 64);
#pragma unroll
      for (int pt = 0; pt < PT16; ++pt) fb[pt] = *reinterpret_cast<const bf16x8*>(pb + boff[pt] + ks * 64);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int pt = 0; pt < PT16; ++pt)
          acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[ct], fb[pt], acc[ct][pt], 0, 0, 0);
    }
  };

  // one chunk = 9 fully unrolled tap steps; PAR = parity of its first step (selects register set / LDS slot)
  auto chunk_body = [&](int c, auto par_tag) {
    constexpr int PAR = decltype(par_tag)::value;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int set = (PAR + tap) & 1;
      store_b(breg[set], set);
      __syncthreads();
      if (tap + 2 < 9 || c + 1 < nchunks) load_b(breg[set], c, tap + 2);   // uniform branch; no loads past the end
      if (tap == 6 && c + 1 < nchunks) load_a(c + 1);
      compute((tap / 3) * C::RS + (tap % 3) * C::PSTR, set);
    }
    if (c + 1 < nchunks) {
      __syncthreads();        // every wave is done with this chunk's patch
      store_a();
    }
  };

  load_a(0);
  load_b(breg[0], 0, 0);
  load_b(breg[1], 0, 1);
  store_a();
  int c = 0;
  for (; c + 1 < nchunks; c += 2) {
    chunk_body(c, std::integral_constant<int, 0>{});
    chunk_body(c + 1, std::integral_constant<int, 1>{});
  }
  if (c < nchunks) chunk_body(c, std::integral_constant<int, 0>{});

  // ---- epilogue: D of 16x16x32: col = lane&15 (pixel), rows (lane>>4)*4 + reg (4 consecutive channels)
  float bs[4][4], bq[4][4];            // BatchNorm partials of this lane: [ct][reg] over its pixels
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int j = 0; j < 4; ++j) { bs[ct][j] = 0.f; bq[ct][j] = 0.f; }
#pragma unroll
  for (int pt = 0; pt < PT16; ++pt) {
    const int fy = ty0 + wpx * PT16 + pt, fx = tx0 + l15;
    if (fy >= P.H || fx >= P.W) continue;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      int co = co0 + wco * 64 + ct * 16 + kb * 4;
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = acc[ct][pt][j];
      if (P.bias) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] += P.bias[co + j];
      }
      if (P.relu) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
      }
      const int accq = (co < P.dst_split) ? (P.accumulate & 1) : (P.accumulate & 2);   // per-view accumulate bit
        const DViewW D = (co < P.dst_split) ? P.dst[0] : P.dst[1];
      if (co >= P.dst_split) co -= P.dst_split;
      const int y = fy - D.oy, x = fx - D.ox;
      if (y < 0 || y >= D.H || x < 0 || x >= D.W) continue;
      T* o = reinterpret_cast<T*>(D.p) + ((size_t)(n * D.H + y) * D.W + x) * D.C + co;
      if (accq) {
        bf16x4 old = *reinterpret_cast<const bf16x4*>(o);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] += (float)old[j];
      }
      bf16x4 r;
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = (bf16_t)v[j];
      *reinterpret_cast<bf16x4*>(o) = r;
#pragma unroll
      for (int j = 0; j < 4; ++j) {              // statistics of the value as STORED (bf16-rounded)
        const float q = (float)r[j];
        bs[ct][j] += q;
        bq[ct][j] = fmaf(q, q, bq[ct][j]);
      }
    }
  }
  if (P.stats) {
    // wavefront reduction over the 16 pixel lanes of each channel group, then the two pixel-waves through LDS
#pragma unroll
    for (int m = 1; m < 16; m <<= 1)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          bs[ct][j] += __shfl_xor(bs[ct][j], m);
          bq[ct][j] += __shfl_xor(bq[ct][j], m);
        }
    __syncthreads();                               // all MFMA operand reads of the tile are done: reuse LDS
    float* red = reinterpret_cast<float*>(smem);   // [WPX][2][BN]
    if (l15 == 0) {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int cl = wco * 64 + ct * 16 + kb * 4 + j;
          red[(wpx * 2 + 0) * BN + cl] = bs[ct][j];
          red[(wpx * 2 + 1) * BN + cl] = bq[ct][j];
        }
    }
    __syncthreads();
    const int part = (n * P.tilesY + tyi) * P.tilesX + txi;
    for (int i = tid; i < 2 * BN; i += 256) {
      const int q = i / BN, cl = i - q * BN;
      float t = 0.f;
#pragma unroll
      for (int wp = 0; wp < C::WPX; ++wp) t += red[(wp * 2 + q) * BN + cl];
      P.stats[((size_t)part * 2 + q) * P.Cout + co0 + cl] = t;
    }
  }
}

template <typename T, int BN, int KG>
int32_t launch3(const IgemmParams& Pin, int kclass, hipStream_t s, int* stat_parts) {
  using C = Cfg3<T, BN, KG>;
  IgemmParams P = Pin;
  const long long blocks = (long long)P.N * P.tilesY * P.tilesX * P.nCo;
  UNET_REQUIRE(blocks > 0 && blocks < (1LL << 31), UNET_ERR_UNSUPPORTED, "conv3: grid of %lld blocks", blocks);
  const double flops = 2.0 * P.N * P.H * P.W * (double)P.Cout * P.Ctot * 9;
  if constexpr (sizeof(T) == 2 && BN == 128 && KG == 4) {
    // the 16x16x32 MFMA variant (up to 7 % faster than the 32x32x16 conv3_kernel in interleaved A/B runs: the chip
    // holds a higher clock on that shape)
    using CM = Cfg3M<T, BN, KG>;
    auto km = conv3m16_kernel<T, BN, KG>;
    unet_set_max_lds(reinterpret_cast<const void*>(km), CM::LDS);
    if (P.stats && stat_parts) *stat_parts = P.N * P.tilesY * P.tilesX;   // epilogue writes the BN partials
    ProfScope prof(kclass, flops, s, "conv3m16_kernel");
    hipLaunchKernelGGL(km, dim3((unsigned)blocks), dim3(256), CM::LDS, s, P);
    return unet_check_launch("conv3m16_kernel");
  } else {
    auto kern = conv3_kernel<T, BN, KG>;
    unet_set_max_lds(reinterpret_cast<const void*>(kern), C::LDS);
    P.stats = nullptr;
    ProfScope prof(kclass, flops, s, "conv3_kernel");
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), C::LDS, s, P);
    return unet_check_launch("conv3_kernel");
  }
}

}  // namespace

template <typename T>
int32_t unet_internal_conv3(const IgemmParams& P, bool big, bool k4, int kclass, hipStream_t s, int* stat_parts) {
  if (big) return k4 ? launch3<T, 128, 4>(P, kclass, s, stat_parts) : launch3<T, 128, 1>(P, kclass, s, stat_parts);
  return k4 ? launch3<T, 64, 4>(P, kclass, s, stat_parts) : launch3<T, 64, 1>(P, kclass, s, stat_parts);
}
template int32_t unet_internal_conv3<bf16_t>(const IgemmParams&, bool, bool, int, hipStream_t, int*);
template int32_t unet_internal_conv3<float>(const IgemmParams&, bool, bool, int, hipStream_t, int*);
