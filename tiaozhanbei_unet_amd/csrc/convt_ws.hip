// convt_ws_kernel<CIN>: weight-stationary streaming kernel for the wide transposed convolutions (up3: 256->128,
// up4: 128->64; AI ~ 85-170 FLOP/B => HBM-bound).  ConvTranspose2d(k2,s2) is ONE GEMM [pixels x CIN] x
// [CIN x 4*Cout] whose rows scatter to the 2x2 sub-positions.  Eight waves each keep 32 of 256 GEMM rows x CIN
// of weights in registers (CIN/16 MFMA A-fragments); 128-pixel input tiles (no halo) stream through an LDS ring
// filled by LDS-DMA; per tile and wave CIN/16 x 4 MFMAs, 16 buffer stores (8 B, bias added), one barrier.
#include "conv_common.h"

namespace {

template <int CIN>
struct CfgTW {
  static constexpr int TP = 128;                               // pixels per tile
  static constexpr int ROWP = CIN / 8 + 1;                      // 16-byte pieces per LDS row (one pad piece)
  static constexpr int RSTR = ROWP * 16;                        // 272 / 528 B: conflict-free ds_read_b128
  static constexpr int PIECES = TP * ROWP;
  static constexpr int NWAVE = 8;
  static constexpr int NINSTR = (PIECES + 63) / 64;
  static constexpr int NDMA = (NINSTR + NWAVE - 1) / NWAVE;
  static constexpr int A_BYTES = NINSTR * 1024;
  static constexpr int NBUF = (CIN <= 128) ? 3 : 2;
  static constexpr int LDS = NBUF * A_BYTES + 1024;
  static constexpr int PXT = TP / 32;                           // 4 MFMA pixel tiles per wave
  static constexpr int KGN = CIN / 16;
  static constexpr int NST = 2 * PXT;                           // 16-byte stores per wave per tile
};

template <int CIN>
__global__ __launch_bounds__(512, 1) void convt_ws_kernel(const ConvTParams P) {
  using C = CfgTW<CIN>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hh = lane >> 5;
  const int rows_total = 4 * P.Cout;
  const int nCg = rows_total / 256;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int cg = slot % nCg, tr = (slot / nCg) * 8 + xcd;
  const int row_lane = cg * 256 + wave * 32 + l31;              // GEMM row = z*Cout + co
  const int t_begin = tr * P.tiles_per_block;
  const int t_end = min(t_begin + P.tiles_per_block, P.tiles);
  if (t_begin >= t_end) return;

  bf16x8 wreg[C::KGN];
  {
    const bf16_t* wp = reinterpret_cast<const bf16_t*>(P.w);
#pragma unroll
    for (int kg = 0; kg < C::KGN; ++kg)
      wreg[kg] = *reinterpret_cast<const bf16x8*>(wp + (size_t)row_lane * CIN + kg * 16 + hh * 8);
    __builtin_amdgcn_s_waitcnt(0x0F70);                          // retire here, not inside the tile loop
  }

  constexpr unsigned OOB = 0xFFFFFFF0u;
  const long long total_px = (long long)P.N * P.H * P.W;
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)P.x, (short)0, (int)std::min<long long>(total_px * CIN * 2, 0x7FFFFFFFLL), 0x00020000);
  const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)P.y, (short)0, (int)std::min<long long>(total_px * 4 * P.Cout * 2, 0x7FFFFFFFLL), 0x00020000);
  typedef __attribute__((address_space(3))) void lds_void;

  // DMA descriptors: piece q = idx*64 + lane -> (pixel row, piece in row); pad piece / beyond the tile = OOB
  int d_row[C::NDMA], d_off[C::NDMA];
#pragma unroll
  for (int j = 0; j < C::NDMA; ++j) {
    const int q = (j * C::NWAVE + wave) * 64 + lane;
    const int row = q / C::ROWP, pc = q - row * C::ROWP;
    d_row[j] = (row < C::TP && pc < CIN / 8) ? row : -1;
    d_off[j] = pc * 16;
  }
  auto dma = [&](int tile, int buf) {
    const long long p0 = (long long)tile * C::TP;
#pragma unroll
    for (int j = 0; j < C::NDMA; ++j) {
      const int idx = j * C::NWAVE + wave;
      const long long px = p0 + d_row[j];
      const bool ok = d_row[j] >= 0 && px < total_px;
      const unsigned vo = ok ? (unsigned)(px * (CIN * 2) + d_off[j]) : OOB;
      char* dst = idx < C::NINSTR ? smem + buf * C::A_BYTES + idx * 1024 : smem + C::NBUF * C::A_BYTES;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (lds_void*)dst, 16, vo, 0, 0, 0);
    }
  };

  float bias4[4][4];                      // bias of this lane's 16 rows: [g][j] -> row 8g + 4hh + j
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = cg * 256 + wave * 32 + 8 * g + 4 * hh + j;
      bias4[g][j] = P.bias ? P.bias[r % P.Cout] : 0.f;
    }
  __builtin_amdgcn_s_waitcnt(0x0F70);

  static_assert(2 * C::NST + C::NDMA * (C::NBUF - 1) <= 63, "vmcnt range");
#pragma unroll
  for (int d = 0; d < C::NBUF - 1; ++d)
    if (t_begin + d < t_end) dma(t_begin + d, d);
  const int HW = P.H * P.W;
  for (int tile = t_begin; tile < t_end; ++tile) {
    const int k = tile - t_begin;
    const int cur = k % C::NBUF;
    // ops younger than tile `tile`'s DMAs: the DMAs of the (NBUF-2) later tiles still in flight + the stores of
    // the previous tiles issued after them (exact counts; see conv3_ws_kernel)
    const int later = min(C::NBUF - 2, t_end - 1 - tile);      // later tiles whose DMAs are already issued
    const int st_tiles = min(k, C::NBUF - 1);                  // previous tiles whose stores are younger
    if constexpr (C::NBUF == 3) {
      // issue order: ... DMA(t) | stores(t-2) | DMA(t+1) | stores(t-1) |  -> younger than DMA(t):
      if (later >= 1) {
        if (st_tiles >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * C::NST + C::NDMA) : "memory");
        else if (st_tiles == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NST + C::NDMA) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NDMA) : "memory");
      } else {
        if (st_tiles >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * C::NST) : "memory");
        else if (st_tiles == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NST) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    } else {
      // NBUF == 2: DMA(t) was issued during tile t-1, before stores(t-1)
      if (st_tiles >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NST) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    if (tile + C::NBUF - 1 < t_end) dma(tile + C::NBUF - 1, (k + C::NBUF - 1) % C::NBUF);

    f32x16 acc[C::PXT];
#pragma unroll
    for (int pt = 0; pt < C::PXT; ++pt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[pt][r] = 0.f;
    const char* pb = smem + cur * C::A_BYTES + l31 * C::RSTR + hh * 16;
    {
      // pixel fragments requested two K-groups ahead of their MFMAs, pinned (see conv3_ws_kernel)
      constexpr int DEPTH = 2;
      bf16x8 ring[DEPTH + 1][C::PXT];
#pragma unroll
      for (int i = 0; i < DEPTH && i < C::KGN; ++i)
#pragma unroll
        for (int pt = 0; pt < C::PXT; ++pt)
          ring[i][pt] = *reinterpret_cast<const bf16x8*>(pb + pt * 32 * C::RSTR + i * 32);
#pragma unroll
      for (int kg = 0; kg < C::KGN; ++kg) {
        if (kg + DEPTH < C::KGN) {
#pragma unroll
          for (int pt = 0; pt < C::PXT; ++pt)
            ring[(kg + DEPTH) % (DEPTH + 1)][pt] =
                *reinterpret_cast<const bf16x8*>(pb + pt * 32 * C::RSTR + (kg + DEPTH) * 32);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int pt = 0; pt < C::PXT; ++pt)
          acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wreg[kg], ring[kg % (DEPTH + 1)][pt], acc[pt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }

    // ---- epilogue: scatter to (2y+zk, 2x+zl); exactly NST buffer stores per wave
#pragma unroll
    for (int pt = 0; pt < C::PXT; ++pt) {
      const long long px = (long long)tile * C::TP + pt * 32 + l31;
      const bool ok = px < total_px;
      const int n = (int)(px / HW), rem = (int)(px - (long long)n * HW);
      const int y = rem / P.W, x = rem - y * P.W;
#pragma unroll
      for (int gp = 0; gp < 2; ++gp) {
        // v_permlane32_swap: the lower half-wave gives its g-odd run for the upper one's g-even run; each lane
        // then owns 8 consecutive rows (16gp + 8hh ..) and writes 16 bytes
        bf16x4 xa, xb;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          xa[j] = (bf16_t)(acc[pt][8 * gp + j] + bias4[2 * gp][j]);
          xb[j] = (bf16_t)(acc[pt][8 * gp + 4 + j] + bias4[2 * gp + 1][j]);
        }
        const u32x2 ua = __builtin_bit_cast(u32x2, xa), ub = __builtin_bit_cast(u32x2, xb);
        const auto s0 = __builtin_amdgcn_permlane32_swap(ua[0], ub[0], false, false);
        const auto s1 = __builtin_amdgcn_permlane32_swap(ua[1], ub[1], false, false);
        const int r = cg * 256 + wave * 32 + 16 * gp + 8 * hh;
        const int z = r / P.Cout, co = r - z * P.Cout;
        const long long opix = ((long long)n * 2 * P.H + 2 * y + (z >> 1)) * (2 * P.W) + 2 * x + (z & 1);
        const unsigned vo = ok ? (unsigned)((opix * P.Cout + co) * 2) : OOB;
        __builtin_amdgcn_raw_buffer_store_b128(u32x4{s0[0], s1[0], s0[1], s1[1]}, yrs, vo, 0, 0);
      }
    }
  }
}

template <int CIN>
int32_t launch_convt_ws(ConvTParams P, hipStream_t s) {
  using C = CfgTW<CIN>;
  auto kern = convt_ws_kernel<CIN>;
  unet_set_max_lds(reinterpret_cast<const void*>(kern), C::LDS);
  const long long total_px = (long long)P.N * P.H * P.W;
  P.tiles = (int)cdiv64(total_px, C::TP);
  const int nCg = 4 * P.Cout / 256;
  int tpb = (int)cdiv64((long long)P.tiles * nCg, unet_cu_budget());
  if (tpb < 2) tpb = 2;
  P.tiles_per_block = tpb;
  const long long ranges8 = cdiv64(cdiv64(P.tiles, tpb), 8) * 8;
  const double flops = 2.0 * total_px * 4.0 * P.Cout * CIN;
  ProfScope prof(UNET_K_CONVT_FWD, flops, s, "convt_ws_kernel");
  hipLaunchKernelGGL(kern, dim3((unsigned)(ranges8 * nCg)), dim3(512), C::LDS, s, P);
  return unet_check_launch("convt_ws_kernel");
}


// ------------------------------------------------------------------------------------------------------
// convt_dgrad_ws_kernel<COUT>: data gradient of the wide transposed convolutions, same streaming design as
// convt_ws_kernel.  dx[p][ci] = sum_{z,co} dy[(2y+zk, 2x+zl)][co] * w[ci][z][co]: GEMM rows = CIN = 2*COUT,
// K = 4*COUT gathered from the 2x2 sub-positions of dy (the gather happens in the DMA's per-lane source address,
// the LDS row of a pixel is its 4*COUT K-vector).  Weights (32 rows x K per wave) live in registers.
template <int COUT>
struct CfgTD {
  static constexpr int CIN = 2 * COUT, K = 4 * COUT;
  static constexpr int TP = (COUT <= 64) ? 128 : 64;
  static constexpr int ROWP = K / 8 + 1;
  static constexpr int RSTR = ROWP * 16;
  static constexpr int PIECES = TP * ROWP;
  static constexpr int NWAVE = 8;
  static constexpr int NINSTR = (PIECES + 63) / 64;
  static constexpr int NDMA = (NINSTR + NWAVE - 1) / NWAVE;
  static constexpr int A_BYTES = NINSTR * 1024;
  static constexpr int NBUF = 2;
  static constexpr int CT_BASE = NBUF * A_BYTES + 1024;         // BNB: [scale | shift | mean][CIN], then the wave exchange
  static constexpr int LDS = CT_BASE + 3 * CIN * 4 + 2 * 2 * CIN * 4;
  static constexpr int RW = CIN / 32;                           // waves along rows (4 or 8)
  static constexpr int PW = NWAVE / RW;                         // waves along pixels (2 or 1)
  static constexpr int PXT = TP / PW / 32;                      // MFMA pixel tiles per wave (2)
  static constexpr int KGN = K / 16;
  static constexpr int NST = 2 * PXT;
};

// BNB: the gradient this kernel produces is d loss / d a of a conv-BatchNorm-ReLU layer (the DoubleConv in front of the
// Up block, src/model.py:14-19 -> :51): the epilogue loads that layer's raw output y with the store offsets, applies the
// ReLU mask relu'(scale*y+shift), stores dz and keeps per-lane running sums of dz and dz*(y-mean) over the block's
// tiles; one cross-lane / cross-wave reduction at the end -> one ordered partial per block (deterministic).
template <int COUT, bool BNB = false>
__global__ __launch_bounds__(512, 1) void convt_dgrad_ws_kernel(const ConvTParams P) {
  using C = CfgTD<COUT>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hh = lane >> 5;
  const int wr = wave % C::RW, wp = wave / C::RW;
  const int row_lane = wr * 32 + l31;
  const int t_begin = blockIdx.x * P.tiles_per_block;
  const int t_end = min(t_begin + P.tiles_per_block, P.tiles);
  if (t_begin >= t_end) {
    if (BNB) for (int i = tid; i < 2 * C::CIN; i += 512) P.stats[(size_t)blockIdx.x * 2 * C::CIN + i] = 0.f;
    return;
  }
  float* const ctab = reinterpret_cast<float*>(smem + C::CT_BASE);
  if constexpr (BNB) {
    for (int i = tid; i < 3 * C::CIN; i += 512)
      ctab[i] = (i < C::CIN ? P.bn_scale : (i < 2 * C::CIN ? P.bn_shift : P.bn_mean))[i % C::CIN];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // (the tile loop's raw barrier does not wait for LDS writes)
  }
  float rs0[2][2][4], rs1[2][2][4];               // BNB: running sums [16-channel group][run][row] of this lane's channels
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int j = 0; j < 4; ++j) { rs0[a][b][j] = 0.f; rs1[a][b][j] = 0.f; }

  bf16x8 wreg[C::KGN];
  {
    const bf16_t* wpk = reinterpret_cast<const bf16_t*>(P.w);
#pragma unroll
    for (int kg = 0; kg < C::KGN; ++kg)
      wreg[kg] = *reinterpret_cast<const bf16x8*>(wpk + (size_t)row_lane * C::K + kg * 16 + hh * 8);
    __builtin_amdgcn_s_waitcnt(0x0F70);
  }

  constexpr unsigned OOB = 0xFFFFFFF0u;
  const long long total_px = (long long)P.N * P.H * P.W;       // dx pixels (half-resolution grid)
  const int HW = P.H * P.W;
  // P.x = dy [N][2H][2W][COUT], P.y = dx [N][H][W][CIN]
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)P.x, (short)0, (int)std::min<long long>(total_px * 4 * COUT * 2, 0x7FFFFFFFLL), 0x00020000);
  const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)P.y, (short)0, (int)std::min<long long>(total_px * C::CIN * 2, 0x7FFFFFFFLL), 0x00020000);
  const __amdgpu_buffer_rsrc_t bnrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(BNB ? P.bn_y : P.x), (short)0, (int)std::min<long long>(total_px * C::CIN * 2, 0x7FFFFFFFLL), 0x00020000);
  (void)bnrs;
  typedef __attribute__((address_space(3))) void lds_void;

  int d_row[C::NDMA], d_z[C::NDMA], d_c[C::NDMA];
#pragma unroll
  for (int j = 0; j < C::NDMA; ++j) {
    const int q = (j * C::NWAVE + wave) * 64 + lane;
    const int row = q / C::ROWP, pc = q - row * C::ROWP;
    d_row[j] = (row < C::TP && pc < C::K / 8) ? row : -1;
    d_z[j] = pc / (COUT / 8);
    d_c[j] = (pc % (COUT / 8)) * 16;
  }
  auto dma = [&](int tile, int buf, bool live = true) {
    const long long p0 = (long long)tile * C::TP;
#pragma unroll
    for (int j = 0; j < C::NDMA; ++j) {
      const int idx = j * C::NWAVE + wave;
      const long long px = p0 + d_row[j];
      const bool ok = live && d_row[j] >= 0 && px < total_px;
      const int n = (int)(px / HW), rem = (int)(px - (long long)n * HW);
      const int y = rem / P.W, x = rem - y * P.W;
      const long long ipix = ((long long)n * 2 * P.H + 2 * y + (d_z[j] >> 1)) * (2 * P.W) + 2 * x + (d_z[j] & 1);
      const unsigned vo = ok ? (unsigned)(ipix * (COUT * 2) + d_c[j]) : OOB;
      char* dst = (live && idx < C::NINSTR) ? smem + buf * C::A_BYTES + idx * 1024 : smem + C::NBUF * C::A_BYTES;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (lds_void*)dst, 16, vo, 0, 0, 0);
    }
  };

  dma(t_begin, 0);
  for (int tile = t_begin; tile < t_end; ++tile) {
    const int k = tile - t_begin;
    const int cur = k & 1;
    // DMA(t) was issued during tile t-1 BEFORE stores(t-1): exactly NST younger ops
    if (k >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NST) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // BNB: this tile's y values (same offsets as the stores) are requested FIRST, then the next tile's DMAs, so that the
    // epilogue's wait for them leaves those DMAs in flight
    u32x4 yv[BNB ? C::PXT : 1][2];
    unsigned ovo[C::PXT][2];
#pragma unroll
    for (int pt = 0; pt < C::PXT; ++pt) {
      const long long px = (long long)tile * C::TP + (wp * C::PXT + pt) * 32 + l31;
#pragma unroll
      for (int gp = 0; gp < 2; ++gp) {
        ovo[pt][gp] = px < total_px ? (unsigned)((px * C::CIN + wr * 32 + 16 * gp + 8 * hh) * 2) : OOB;
        // (inline asm: hipcc does not count LDS-DMA instructions, so its own wait for a builtin load issued in front of
        //  the next tile's DMAs would be vmcnt(3) -- draining those DMAs every tile; the wait is hand-counted below)
        if constexpr (BNB)
          asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(yv[pt][gp]) : "v"(ovo[pt][gp]), "s"(bnrs) : "memory");
      }
    }
    if (BNB || tile + 1 < t_end) dma(tile + 1, cur ^ 1, tile + 1 < t_end);   // (BNB: always NDMA instructions -> one wait form)

    f32x16 acc[C::PXT];
#pragma unroll
    for (int pt = 0; pt < C::PXT; ++pt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[pt][r] = 0.f;
    const char* pb = smem + cur * C::A_BYTES + (wp * C::PXT * 32 + l31) * C::RSTR + hh * 16;
    {
      // pixel fragments requested two K-groups ahead of their MFMAs, pinned (see conv3_ws_kernel)
      constexpr int DEPTH = BNB ? 1 : 2;            // (the fused form needs the registers for its sums and y values)
      bf16x8 ring[DEPTH + 1][C::PXT];
#pragma unroll
      for (int i = 0; i < DEPTH && i < C::KGN; ++i)
#pragma unroll
        for (int pt = 0; pt < C::PXT; ++pt)
          ring[i][pt] = *reinterpret_cast<const bf16x8*>(pb + pt * 32 * C::RSTR + i * 32);
#pragma unroll
      for (int kg = 0; kg < C::KGN; ++kg) {
        if (kg + DEPTH < C::KGN) {
#pragma unroll
          for (int pt = 0; pt < C::PXT; ++pt)
            ring[(kg + DEPTH) % (DEPTH + 1)][pt] =
                *reinterpret_cast<const bf16x8*>(pb + pt * 32 * C::RSTR + (kg + DEPTH) * 32);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int pt = 0; pt < C::PXT; ++pt)
          acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wreg[kg], ring[kg % (DEPTH + 1)][pt], acc[pt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if constexpr (BNB) {
      // the y loads are older than the next tile's DMAs: leave exactly those in flight
      static_assert(C::PXT == 2, "wait statement names 4 destinations");
      asm volatile("s_waitcnt vmcnt(%4)" : "+v"(yv[0][0]), "+v"(yv[0][1]), "+v"(yv[1][0]), "+v"(yv[1][1]) : "n"(C::NDMA));
    }
#pragma unroll
    for (int pt = 0; pt < C::PXT; ++pt) {
#pragma unroll
      for (int gp = 0; gp < 2; ++gp) {               // 16-byte stores (see convt_ws_kernel)
        bf16x4 xa, xb;
        if constexpr (BNB) {
          // y comes in with the store's 8-consecutive-channel layout: un-swap it to the accumulator's two 4-row runs
          const u32x4 o = yv[pt][gp];
          const auto o0 = __builtin_amdgcn_permlane32_swap(o[0], o[2], false, false);
          const auto o1 = __builtin_amdgcn_permlane32_swap(o[1], o[3], false, false);
          const bf16x4 ya = __builtin_bit_cast(bf16x4, u32x2{o0[0], o1[0]});
          const bf16x4 yb = __builtin_bit_cast(bf16x4, u32x2{o0[1], o1[1]});
          const bool ok = ovo[pt][gp] != OOB;
          const int cb = wr * 32 + 16 * gp + 4 * hh;
          const f32x4 sca = *reinterpret_cast<const f32x4*>(ctab + cb), scb = *reinterpret_cast<const f32x4*>(ctab + cb + 8);
          const f32x4 sha = *reinterpret_cast<const f32x4*>(ctab + C::CIN + cb);
          const f32x4 shb = *reinterpret_cast<const f32x4*>(ctab + C::CIN + cb + 8);
          const f32x4 mua = *reinterpret_cast<const f32x4*>(ctab + 2 * C::CIN + cb);
          const f32x4 mub = *reinterpret_cast<const f32x4*>(ctab + 2 * C::CIN + cb + 8);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float fa = (float)ya[j], fb = (float)yb[j];
            xa[j] = (bf16_t)((ok && fmaf(fa, sca[j], sha[j]) > 0.f) ? acc[pt][8 * gp + j] : 0.f);
            xb[j] = (bf16_t)((ok && fmaf(fb, scb[j], shb[j]) > 0.f) ? acc[pt][8 * gp + 4 + j] : 0.f);
            const float qa = (float)xa[j], qb = (float)xb[j];                // dz as stored
            rs0[gp][0][j] += qa;
            rs1[gp][0][j] = fmaf(qa, fa - mua[j], rs1[gp][0][j]);
            rs0[gp][1][j] += qb;
            rs1[gp][1][j] = fmaf(qb, fb - mub[j], rs1[gp][1][j]);
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) { xa[j] = (bf16_t)acc[pt][8 * gp + j]; xb[j] = (bf16_t)acc[pt][8 * gp + 4 + j]; }
        }
        const u32x2 ua = __builtin_bit_cast(u32x2, xa), ub = __builtin_bit_cast(u32x2, xb);
        const auto s0 = __builtin_amdgcn_permlane32_swap(ua[0], ub[0], false, false);
        const auto s1 = __builtin_amdgcn_permlane32_swap(ua[1], ub[1], false, false);
        __builtin_amdgcn_raw_buffer_store_b128(u32x4{s0[0], s1[0], s0[1], s1[1]}, yrs, ovo[pt][gp], 0, 0);
      }
    }
  }
  if constexpr (BNB) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // (the last tile's dummy DMAs)
    // the block's partial: sums over the 32 pixel lanes of a half-wave (fixed butterfly order), then over the PW pixel
    // waves through LDS, one store per (statistic, channel)
    float* ex = ctab + 3 * C::CIN;                  // [PW][2][CIN]
#pragma unroll
    for (int gp = 0; gp < 2; ++gp)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float a = rs0[gp][t][j], b = rs1[gp][t][j];
#pragma unroll
          for (int m = 1; m < 32; m <<= 1) { a += __shfl_xor(a, m); b += __shfl_xor(b, m); }
          if (l31 == 0) {
            const int ch = wr * 32 + 16 * gp + 8 * t + 4 * hh + j;
            ex[(wp * 2 + 0) * C::CIN + ch] = a;
            ex[(wp * 2 + 1) * C::CIN + ch] = b;
          }
        }
    __syncthreads();
    for (int i = tid; i < 2 * C::CIN; i += 512) {
      float t = 0.f;
#pragma unroll
      for (int w2 = 0; w2 < C::PW; ++w2) t += ex[(w2 * 2 + i / C::CIN) * C::CIN + i % C::CIN];
      P.stats[(size_t)blockIdx.x * 2 * C::CIN + i] = t;
    }
  }
}

template <int COUT>
int32_t launch_convt_dgrad_ws(ConvTParams P, hipStream_t s, int* n_parts = nullptr) {
  using C = CfgTD<COUT>;
  const bool bnb = P.bn_y != nullptr;
  auto kern = (bnb && COUT == 64) ? convt_dgrad_ws_kernel<COUT, (COUT == 64)> : convt_dgrad_ws_kernel<COUT, false>;
  unet_set_max_lds(reinterpret_cast<const void*>(kern), C::LDS);
  const long long total_px = (long long)P.N * P.H * P.W;
  P.tiles = (int)cdiv64(total_px, C::TP);
  int tpb = (int)cdiv64(P.tiles, std::min(256, unet_cu_budget()));     // (partial buffer: 256 parts)
  if (tpb < 2) tpb = 2;
  P.tiles_per_block = tpb;
  const long long blocks = cdiv64(P.tiles, tpb);
  if (n_parts) *n_parts = (int)blocks;
  const double flops = 2.0 * total_px * 4.0 * COUT * C::CIN;
  ProfScope prof(UNET_K_CONVT_DGRAD, flops, s, bnb ? "convt_dgrad_ws_bnbwd_kernel" : "convt_dgrad_ws_kernel");
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(512), C::LDS, s, P);
  return unet_check_launch("convt_dgrad_ws_kernel");
}

}  // namespace

int32_t unet_internal_convt_ws(int c_in, ConvTParams P, hipStream_t s) {
  return c_in == 128 ? launch_convt_ws<128>(P, s) : launch_convt_ws<256>(P, s);
}

int32_t unet_internal_convt_dgrad_ws(int c_out, ConvTParams P, hipStream_t s, int* n_parts) {
  return c_out == 64 ? launch_convt_dgrad_ws<64>(P, s, n_parts) : launch_convt_dgrad_ws<128>(P, s, n_parts);
}
