// conv3_ws_kernel: weight-stationary 3x3 convolution for the wide-spatial / narrow-channel layers
// (64 input channels: inc.*, up4.conv.3, their data gradients, the 128-row dgrad of up4.conv.0).
// These layers are HBM-bound (AI ~ 288 FLOP/B at bf16), their whole filter bank is tiny (9*64*Cout bf16),
// and the per-tap weight staging + barrier of the generic kernel dominated their run time.  Here every
// wave keeps ITS 32 output channels x 576 K of weights in REGISTERS (36 MFMA A-fragments = 144 VGPRs,
// loaded once per block straight from global memory) and the block streams pixel tiles: the halo'd patch
// of tile t+1 is prefetched (buffer loads -> registers) while tile t computes and lands in the other LDS
// buffer; one barrier per tile, no weight traffic through LDS at all, 72 MFMAs per wave between barriers.
#include "conv_common.h"

namespace {

struct CfgWS {
  static constexpr int WTH = 16, WTW = 16;                      // 256-pixel tiles: halo overhead 1.27x
  static constexpr int HH = WTH + 2, HW = WTW + 2;
  static constexpr int PSTR = 128 + 16;
  static constexpr int RS = (HW * PSTR + 255) / 256 * 256;
  static constexpr int PIECES = HH * (RS / 16);                 // 16-byte pieces of the padded image (pads included)
  static constexpr int NWAVE = 8;                               // 512 threads: 2 (channels) x 4 (pixels)
  static constexpr int NINSTR = (PIECES + 63) / 64;             // 1 KiB LDS-DMA instructions per patch
  static constexpr int NDMA = (NINSTR + NWAVE - 1) / NWAVE;     // per wave per tile (surplus ones hit a dummy KiB)
  static constexpr int A_BYTES = NINSTR * 1024;
  static constexpr int NBUF = 3;                                // patch ring: 2 tiles in flight behind the one computing
  static constexpr int RED_BASE = NBUF * A_BYTES + 1024;        // (+ dummy target of the surplus (all-OOB) DMAs)
  static constexpr int RED_BYTES = 2 * 2 * 8 * 64 * 4;          // [2 tiles][2 statistics][8 half-wave slots][64 channels]
  static constexpr int CT_BASE = RED_BASE + RED_BYTES;          // BatchNorm coefficients of the fused backward mask
  static constexpr int LDS = CT_BASE + 3 * 64 * 4;
  static constexpr int PXT = 2;                                 // 64 pixels per wave
  static constexpr int ROWS = 64;                               // output channels per block
};

// STATS: 0 none; 1 = BatchNorm batch statistics of the stored outputs (sum, sum of squares: the forward of
// conv -> BatchNorm, no separate pass over y); 2 = data gradient with the ReLU mask of the producing layer and its
// BatchNorm-backward sums (sum dz, sum dz * (y - mean); see IgemmParams::bn_y).  A wave cannot afford per-lane running
// sums next to its 144 weight registers, so every tile's 2 x 16 per-lane values are reduced over the 16 lanes of a DPP
// row at once (4 VALU adds each), the four row leaders leave them in an LDS slot, and 128 threads keep the block's
// running total of their (statistic, channel) -- one ordered partial per block: deterministic.
// ST ("stagger", the statistics form STATS == 1): a tile is two phases with a barrier after each -- M: the DMA issue of
// the tile two ahead + the 72 MFMAs (+ the counted wait for the NEXT tile's patch), E: the tile's epilogue (pack,
// statistics, stores) + the next tile's output geometry -- and waves 4-7 run one barrier behind waves 0-3, so on every SIMD one wave's MFMA phase
// covers its partner's VALU/store phase (in lock-step all eight did their epilogues together, then fought over the
// matrix pipe: 40 % MFMA busy).  Waves 0-3 own output channels 0-31, waves 4-7 channels 32-63 (a half's statistics
// stay inside the half).  It pays where the epilogue is long (+3.5 % on 64 -> 64 @256x256) and costs 20 % where it is
// short (plain forward / data gradient: the DMA burst of a half then lands inside the other half's MFMA phase).
template <bool ACC, int STATS = 0>
__global__ __launch_bounds__(512, 1) void conv3_ws_kernel(const IgemmParams P, int tiles_per_block) {
  using C = CfgWS;
  constexpr bool ST = STATS == 1;
  static_assert(!(ACC && STATS), "the gradient fan-in form carries no statistics");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = wave >> 2;
  const int wco = ST ? grp : (wave & 1), wpx = ST ? (wave & 3) : (wave >> 1);
  const int l31 = lane & 31, hh = lane >> 5;
  const int nCg = P.Cout / C::ROWS;
  // channel groups of one tile range sit on the SAME XCD (b % 8) in adjacent dispatch slots, so the
  // second group finds the patches in that XCD's L2
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int cg = slot % nCg, tr = (slot / nCg) * 8 + xcd;
  const int co_lane = cg * C::ROWS + wco * 32 + l31;
  const int tiles_img = P.tilesX * P.tilesY;
  const int total_tiles = P.N * tiles_img;
  const int t_begin = tr * tiles_per_block;
  const int t_end = min(t_begin + tiles_per_block, total_tiles);
  if (t_begin >= t_end) {
    if (STATS && tid < 128)                       // an empty tile range still owns a partial: zeros
      P.stats[((size_t)tr * 2 + (tid >> 6)) * P.Cout + cg * C::ROWS + (tid & 63)] = 0.f;
    return;
  }
  float* const red = reinterpret_cast<float*>(smem + C::RED_BASE);
  float* const ctab = reinterpret_cast<float*>(smem + C::CT_BASE);      // [scale | shift | mean][64]
  if (STATS == 2 && tid < 192) {
    const float* srcp = tid < 64 ? P.bn_scale : (tid < 128 ? P.bn_shift : P.bn_mean);
    ctab[tid] = srcp[cg * C::ROWS + (tid & 63)];
  }
  float stat_tot = 0.f;

  // ---- this wave's weights -> registers: A fragment (tap, kg) = W[co_lane][tap][16*kg + 8*hh .. +7]
  bf16x8 wreg[36];
  {
    const bf16_t* wp = reinterpret_cast<const bf16_t*>(P.w);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int kg = 0; kg < 4; ++kg)
        wreg[tap * 4 + kg] = *reinterpret_cast<const bf16x8*>(wp + ((size_t)(tap * P.Cout + co_lane)) * P.wK + kg * 16 + hh * 8);
    // retire the weight loads HERE (vmcnt(0)), through the builtin so hipcc's wait bookkeeping sees it:
    // otherwise it places counted waits for them inside the tile loop, which would drain the DMA ring.
    __builtin_amdgcn_s_waitcnt(0x0F70);
  }

  int boff[C::PXT];
#pragma unroll
  for (int pt = 0; pt < C::PXT; ++pt) {
    const int m = wpx * (32 * C::PXT) + pt * 32 + l31;
    boff[pt] = (m >> 4) * C::RS + (m & 15) * C::PSTR + hh * 16;
  }
  constexpr unsigned OOB = 0xFFFFFFF0u;
  const DView S = P.src[0];
  // LDS-DMA staging (buffer_load_dwordx4 ... lds): the padded LDS image is filled LINEARLY, 1 KiB per wave
  // instruction; pad pieces and out-of-image halo pixels use an out-of-range voffset and land as zeros.
  // No staging registers: whole patches are in flight while this tile computes.
  // per lane and instruction, constant over the tiles, two to a register: hy | hx << 5 | piece << 10 | 1 << 14 (0 = pad
  // piece).  A tile then costs a dozen VALU instructions per DMA (the tile's own origin is scalar) where the lane
  // geometry used to be divided out and multiplied up per tile (~300 per tile, fighting the partner wave's epilogue for
  // the SIMD's vector issue: the stamps showed them taking as long as the tile's 72 MFMAs).
  unsigned a_pk[(C::NDMA + 1) / 2];
#pragma unroll
  for (int j = 0; j < C::NDMA; ++j) {
    const int q = (j * C::NWAVE + wave) * 64 + lane;              // instruction index j*NWAVE + wave
    const int hy = q / (C::RS / 16), rem = q - hy * (C::RS / 16);
    const int hx = rem / 9, part = rem - hx * 9;
    const unsigned code = (hy < C::HH && hx < C::HW && part < 8) ? (unsigned)(hy | (hx << 5) | (part << 10) | (1 << 14)) : 0u;
    if (j & 1) a_pk[j >> 1] |= code << 16;
    else a_pk[j >> 1] = code;
  }
  const unsigned img_bytes = (unsigned)S.H * S.W * S.C * 2u;
  typedef __attribute__((address_space(3))) void lds_void;

  // tile coordinates advance by increments (no per-tile divisions): one iterator per consumer
  struct TileIt { int n, ty, tx; };
  auto tile_at = [&](int tile) {
    TileIt it;
    it.n = tile / tiles_img;
    const int r = tile - it.n * tiles_img;
    it.ty = r / P.tilesX;
    it.tx = r - it.ty * P.tilesX;
    return it;
  };
  auto tile_next = [&](TileIt& it) {
    if (++it.tx == P.tilesX) {
      it.tx = 0;
      if (++it.ty == P.tilesY) { it.ty = 0; ++it.n; }
    }
  };
  TileIt dma_it = tile_at(t_begin), geo_it = dma_it;

  auto dma_a = [&](int buf, bool live) {         // the patch of the tile at dma_it (then advance); dead = to the dummy KiB
    const int ym1 = dma_it.ty * C::WTH - 1, xm1 = dma_it.tx * C::WTW - 1;
    const unsigned base = (unsigned)((ym1 * S.W + xm1) * S.C * 2);      // (may wrap below zero: only valid sums are used)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(S.p + (size_t)(live ? dma_it.n : 0) * img_bytes), (short)0, (int)img_bytes, 0x00020000);
#pragma unroll
    for (int j = 0; j < C::NDMA; ++j) {
      unsigned code = (a_pk[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu;
      asm volatile("" : "+v"(code));               // decode per tile: hoisted out of the loop it costs 21 live registers
      const int hy = code & 31, hx = (code >> 5) & 31, part = (code >> 10) & 15;
      const unsigned y = (unsigned)(ym1 + hy), x = (unsigned)(xm1 + hx);
      const bool ok = live && (code >> 14) && y < (unsigned)S.H && x < (unsigned)S.W;
      const unsigned vo = ok ? base + (unsigned)((hy * S.W + hx) * S.C * 2 + part * 16) : OOB;
      const int idx = j * C::NWAVE + wave;                          // wave-uniform
      char* dst = (live && idx < C::NINSTR) ? smem + buf * C::A_BYTES + idx * 1024 : smem + C::NBUF * C::A_BYTES;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)dst, 16, vo, 0, 0, 0);
    }
    tile_next(dma_it);
  };

  // ring of NBUF patches: tile k computes from slot k % NBUF while the DMAs of tiles k+1, k+2 are in flight.
  // Waits are COUNTED.  vmcnt counts loads, DMAs and stores in issue order; per tile every wave issues
  // exactly NDMA DMAs and NST stores (out-of-range ones are buffer ops with an OOB offset: issued, counted,
  // dropped by the range check), so the ops younger than tile j's DMAs are known exactly:
  //   stores(j-2) + DMA(j+1) + stores(j-1)  ->  vmcnt(2*NST + NDMA) retires tile j's patch while the next
  //   patch and 32 stores stay in flight.  Raw s_barrier (a __syncthreads() here would emit vmcnt(0)).
  constexpr int NVIEW = STATS ? 1 : 2;           // the statistics forms write ONE dense destination
  constexpr int NST = 2 * C::PXT * NVIEW;        // stores per wave per tile: 2 sixteen-channel groups x PXT x dst views
  // STATS == 2 adds NY loads of y per tile, issued BEFORE the tile's DMAs (so that waiting for them in the epilogue
  // leaves those DMAs in flight); by the next tile's wait they are long complete but still count as issued-after
  constexpr int NY = STATS == 2 ? 2 * C::PXT : 0;
  static_assert(2 * NST + C::NDMA + NY <= 63, "vmcnt range");
  // ---- output geometry of a tile (buffer stores: an OOB offset = dropped, so the op count is static)
  // A lane of the 32x32 accumulator owns rows 8g+4hh..+3 of pixel l31; v_permlane32_swap trades the g-odd run
  // of the lower half-wave for the g-even run of the upper one, so every lane ends up with 8 CONSECUTIVE
  // channels (rows 16gp + 8hh ..+7) and writes 16 bytes: half as many store instructions, 32-byte segments.
  __amdgpu_buffer_rsrc_t drs[2];
  unsigned ovo[C::PXT][2][NVIEW];
  int n_img = 0;
  auto geometry = [&]() {                        // of the tile at geo_it (then advance)
    const int n = geo_it.n;
    const int ty0 = geo_it.ty * C::WTH, tx0 = geo_it.tx * C::WTW;
    tile_next(geo_it);
    n_img = n;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const DViewW D = P.dst[q];
      const unsigned dimg = (unsigned)D.H * D.W * D.C * 2u;
      drs[q] = __builtin_amdgcn_make_buffer_rsrc((void*)(D.p ? D.p + (size_t)n * dimg : P.dst[0].p), (short)0,
                                                 D.p ? (int)dimg : 0, 0x00020000);
    }
#pragma unroll
    for (int pt = 0; pt < C::PXT; ++pt) {
      const int m = wpx * (32 * C::PXT) + pt * 32 + l31;
      const int fy = ty0 + (m >> 4), fx = tx0 + (m & 15);
      const bool pix_ok = fy < P.H && fx < P.W;
#pragma unroll
      for (int gp = 0; gp < 2; ++gp) {
        const int co = cg * C::ROWS + wco * 32 + 16 * gp + 8 * hh;
#pragma unroll
        for (int q = 0; q < NVIEW; ++q) {             // one store per destination view; the other one is OOB
          const DViewW D = P.dst[q];
          const int cq = q == 0 ? co : co - P.dst_split;
          const bool mine = (q == 0) == (co < P.dst_split);
          const int y = fy - D.oy, x = fx - D.ox;
          const bool ok = mine && pix_ok && D.p && y >= 0 && y < D.H && x >= 0 && x < D.W;
          ovo[pt][gp][q] = ok ? (unsigned)(((y * D.W + x) * D.C + cq) * 2) : OOB;
        }
      }
    }
  };
  // statistics: the slots of tile kk (this half's four waves, or all eight in lock-step) -> the thread's running total
  const int st_u = ST ? (tid & 255) : tid;
  const bool st_on = STATS && st_u < (ST ? 64 : 128);
  const int st_q = ST ? (st_u >> 5) : (st_u >> 6), st_c = ST ? grp * 32 + (st_u & 31) : (st_u & 63);
  auto take_slots = [&](int kk) {
    if (st_on) {
      const float* rp = red + (kk & 1) * 1024 + st_q * 512 + st_c;
#pragma unroll
      for (int sl = 0; sl < 8; ++sl) stat_tot += rp[sl * 64];
    }
  };

#pragma unroll
  for (int d = 0; d < C::NBUF - 1; ++d)
    if (ST || STATS == 2 || t_begin + d < t_end) dma_a(d, t_begin + d < t_end);
  if constexpr (ST) {
    geometry();
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NDMA) : "memory");          // the first patch; the second one flies
    __builtin_amdgcn_s_barrier();
    if (grp) __builtin_amdgcn_s_barrier();                                  // the stagger
  }
  for (int tile = t_begin; tile < t_end; ++tile) {
    const int k = tile - t_begin;
    const int cur = k % C::NBUF;
    const bool next_in_flight = tile + 1 < t_end;
    if constexpr (!ST) {
    if (k >= 2) {
      if (next_in_flight) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NST + C::NDMA + NY) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NST) : "memory");
    } else if (k == 1) {
      if (next_in_flight) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NST + C::NDMA + NY) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NST) : "memory");
    } else {
      if (next_in_flight) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NDMA) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    if (k >= 1) take_slots(k - 1);                 // the previous tile's slots -> this thread's running total
    geometry();
    }
    const int n = n_img;
    (void)n;
    // STATS == 2: this tile's y values (same offsets as the stores: dst[0] is dense and frame-sized) are requested
    // FIRST, then the DMAs of the tile two ahead
    u32x4 yv[STATS == 2 ? C::PXT : 1][2];
    if constexpr (STATS == 2) {
      const unsigned dimg = (unsigned)P.dst[0].H * P.dst[0].W * P.dst[0].C * 2u;
      const __amdgpu_buffer_rsrc_t yrs =
          __builtin_amdgcn_make_buffer_rsrc((void*)(P.bn_y + (size_t)n * dimg), (short)0, (int)dimg, 0x00020000);
#pragma unroll
      for (int pt = 0; pt < C::PXT; ++pt)
#pragma unroll
        for (int gp = 0; gp < 2; ++gp)     // inline asm + the hand-counted wait below: hipcc does not count LDS-DMA
                                           // instructions, its own wait for a builtin load here would drain the DMA ring
          asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(yv[pt][gp]) : "v"(ovo[pt][gp][0]), "s"(yrs) : "memory");
    }
    // (the statistics-2 form always issues its NDMA instructions -- dead ones to the dummy KiB -- so that one wait form
    //  covers every tile)
    if (ST || STATS == 2 || tile + C::NBUF - 1 < t_end) dma_a((k + C::NBUF - 1) % C::NBUF, tile + C::NBUF - 1 < t_end);
    // gradient fan-in (ACC): the old values are fetched NOW, behind the tile's 72 MFMAs (one load per output
    // run, from whichever view owns it and has its accumulate bit set; everything else reads as 0)
    u32x4 oldv[ACC ? C::PXT : 1][2];
    if constexpr (ACC) {
#pragma unroll
      for (int pt = 0; pt < C::PXT; ++pt)
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) {
          const bool second = ovo[pt][gp][0] == OOB;
          const bool want = (P.accumulate >> (second ? 1 : 0)) & 1;
          const unsigned vo = want ? (second ? ovo[pt][gp][NVIEW - 1] : ovo[pt][gp][0]) : OOB;
          oldv[pt][gp] = second ? __builtin_amdgcn_raw_buffer_load_b128(drs[1], vo, 0, 0)
                                : __builtin_amdgcn_raw_buffer_load_b128(drs[0], vo, 0, 0);
        }
    }

    f32x16 acc[C::PXT];
#pragma unroll
    for (int pt = 0; pt < C::PXT; ++pt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[pt][r] = 0.f;
    const char* pb = smem + cur * C::A_BYTES;
    // 36 (tap, 16-channel group) steps of PXT MFMAs; the pixel fragments of step i+2 are requested before the MFMAs
    // of step i and pinned there (left alone, hipcc requests them one MFMA ahead: the LDS round trip showed)
    constexpr int DEPTH = STATS == 2 ? 1 : 2;             // (the masked-gradient form needs the registers for its y values)
    auto frag = [&](int i, int pt) {
      const int tap = i >> 2, kg = i & 3;
      return *reinterpret_cast<const bf16x8*>(pb + boff[pt] + (tap / 3) * C::RS + (tap % 3) * C::PSTR + kg * 32);
    };
    bf16x8 ring[DEPTH + 1][C::PXT];
#pragma unroll
    for (int i = 0; i < DEPTH; ++i)
#pragma unroll
      for (int pt = 0; pt < C::PXT; ++pt) ring[i][pt] = frag(i, pt);
#pragma unroll
    for (int i = 0; i < 36; ++i) {
      if (i + DEPTH < 36) {
#pragma unroll
        for (int pt = 0; pt < C::PXT; ++pt) ring[(i + DEPTH) % (DEPTH + 1)][pt] = frag(i + DEPTH, pt);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int pt = 0; pt < C::PXT; ++pt)
        acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wreg[i], ring[i % (DEPTH + 1)][pt], acc[pt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }

    if constexpr (STATS == 2) {
      static_assert(C::PXT == 2, "the wait statement names 4 destinations");
      // the y loads are older than this tile's NDMA instructions: exactly those stay in flight
      asm volatile("s_waitcnt vmcnt(%4)" : "+v"(yv[0][0]), "+v"(yv[0][1]), "+v"(yv[1][0]), "+v"(yv[1][1]) : "n"(C::NDMA));
    }
    if constexpr (ST) {
      // end of the M phase: the NEXT tile's patch (issued one tile ago) has landed; younger than it: the previous
      // tile's stores, this tile's y loads and the patch just issued
      if (k >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NST + NY + C::NDMA) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NY + C::NDMA) : "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- epilogue for this tile: exactly NST buffer stores per wave (OOB offset = dropped).  Per 16-channel group gp
    // the two 4-row runs of a lane (t = 0: rows 16gp+4hh.., t = 1: +8) are finished one after the other so that only
    // one run's coefficients and sums are live (the statistics forms sit at the 256-register limit).
#pragma unroll
    for (int gp = 0; gp < 2; ++gp) {
      u32x2 pk[C::PXT][2];                         // packed bf16x4 results: [pixel tile][run]
      u32x2 inp[C::PXT][2];                        // ACC: old values / STATS 2: y, in the accumulator's lane layout
      if constexpr (ACC || STATS == 2) {
#pragma unroll
        for (int pt = 0; pt < C::PXT; ++pt) {
          const u32x4 o = ACC ? oldv[pt][gp] : yv[pt][gp];
          const auto o0 = __builtin_amdgcn_permlane32_swap(o[0], o[2], false, false);
          const auto o1 = __builtin_amdgcn_permlane32_swap(o[1], o[3], false, false);
          inp[pt][0] = u32x2{o0[0], o1[0]};
          inp[pt][1] = u32x2{o0[1], o1[1]};
        }
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float s0[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f};
        f32x4 csc, csh, cmu;
        if constexpr (STATS == 2) {
          const int cb = wco * 32 + 16 * gp + 4 * hh + 8 * t;
          csc = *reinterpret_cast<const f32x4*>(ctab + cb);
          csh = *reinterpret_cast<const f32x4*>(ctab + 64 + cb);
          cmu = *reinterpret_cast<const f32x4*>(ctab + 128 + cb);
        }
#pragma unroll
        for (int pt = 0; pt < C::PXT; ++pt) {
          float f[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) f[j] = acc[pt][8 * gp + 4 * t + j];
          bf16x4 x;
          if constexpr (ACC) {
            const bf16x4 o = __builtin_bit_cast(bf16x4, inp[pt][t]);
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = (bf16_t)(f[j] + (float)o[j]);      // add in fp32, round once
          } else if constexpr (STATS == 2) {
            const bf16x4 yq = __builtin_bit_cast(bf16x4, inp[pt][t]);
            const bool ok = ovo[pt][gp][0] != OOB;                                // a tile pixel outside the frame: no sums
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float yy = (float)yq[j];
              x[j] = (bf16_t)((ok && fmaf(yy, csc[j], csh[j]) > 0.f) ? f[j] : 0.f);
              const float q = (float)x[j];                                        // dz as stored
              s0[j] += q;
              s1[j] = fmaf(q, yy - cmu[j], s1[j]);
            }
          } else {
            if (P.bias) {                            // inference: BatchNorm shift (+ ReLU) of the folded layer
              const float* bp = P.bias + cg * C::ROWS + wco * 32 + 16 * gp + 4 * hh + 8 * t;
#pragma unroll
              for (int j = 0; j < 4; ++j) f[j] += bp[j];
            }
            if (P.relu) {
#pragma unroll
              for (int j = 0; j < 4; ++j) f[j] = fmaxf(f[j], 0.f);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = (bf16_t)f[j];
            if constexpr (STATS == 1) {
              const bool ok = ovo[pt][gp][0] != OOB;
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const float q = ok ? (float)x[j] : 0.f;                           // the value as stored
                s0[j] += q;
                s1[j] = fmaf(q, q, s1[j]);
              }
            }
          }
          pk[pt][t] = __builtin_bit_cast(u32x2, x);
        }
        if constexpr (STATS != 0) {
          float* rw = red + (k & 1) * 1024 + (wpx * 2 + ((lane >> 4) & 1)) * 64 + wco * 32 + 16 * gp + 4 * hh + 8 * t;
          float rv[8];
#pragma unroll
          for (int j = 0; j < 4; ++j) { rv[j] = s0[j]; rv[4 + j] = s1[j]; }
          row16_sum_n(rv);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if ((lane & 15) == 0) { rw[j] = rv[j]; rw[512 + j] = rv[4 + j]; }
        }
      }
#pragma unroll
      for (int pt = 0; pt < C::PXT; ++pt) {
        const auto s0w = __builtin_amdgcn_permlane32_swap(pk[pt][0][0], pk[pt][1][0], false, false);
        const auto s1w = __builtin_amdgcn_permlane32_swap(pk[pt][0][1], pk[pt][1][1], false, false);
        const u32x4 bits = u32x4{s0w[0], s1w[0], s0w[1], s1w[1]};
#pragma unroll
        for (int q = 0; q < NVIEW; ++q) __builtin_amdgcn_raw_buffer_store_b128(bits, drs[q], ovo[pt][gp][q], 0, 0);
      }
    }
    if constexpr (ST) {
      // rest of the E phase: the previous tile's slots (written a barrier pair ago), the next tile's geometry
      if (k >= 1) take_slots(k - 1);
      if (next_in_flight) geometry();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // this tile's slot writes, before the half's barrier
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  if constexpr (ST) { if (!grp) __builtin_amdgcn_s_barrier(); }    // pairs with the stagger barrier of waves 4-7
  if constexpr (STATS != 0) {
    // the last tile's slots, then ONE partial per block
    if constexpr (!ST) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    take_slots(t_end - 1 - t_begin);
    if (st_on) P.stats[((size_t)tr * 2 + st_q) * P.Cout + cg * C::ROWS + st_c] = stat_tot;
  }
  if constexpr (ST || STATS == 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // drain the dummy DMAs before the wave ends
}

// ------------------------------------------------------------------------------------------------------
// conv3_ws16_kernel: the weight-stationary kernel on v_mfma_f32_16x16x32_bf16 (round 2).  Same work split as
// conv3_ws_kernel (8 waves = 2 channel halves x 4 pixel rows-of-4, a wave keeps 32 output channels x 576 K of weights in
// 144 VGPRs, 16x16-pixel tiles stream through a 3-slot LDS-DMA ring, counted vmcnt, one barrier per tile), but
//  * 8 accumulator tiles (2 channel x 4 pixel) of 16x16 per wave instead of 2 of 32x32: eight independent MFMA chains
//    (the 32x32x16 form had two, each MFMA waiting for the one two back: 64-cycle latency at a 32-cycle issue rate) and
//    the shape the chip clocks higher on (MI355X_MICROARCH "DVFS give-back" item 7): a timing-only swap of the
//    instruction measured 208 -> 154 us on 64 -> 64 @256x256;
//  * the LDS patch is UNPADDED (18 x 18 pixels x 128 B, 41 instead of 50 one-KiB DMA instructions per tile), 16-byte
//    pieces XOR-swizzled by (pixel index & 7) through the DMA's per-lane source address: a 16x16x32 pixel fragment
//    (lanes = 16 consecutive pixels x 4 piece columns) is conflict-free for every start pixel; the swizzle term of a
//    read depends on (2 * (pixel row + tap row) + tap column) & 7 only, so 8 per-lane base addresses + immediates cover
//    all 72 reads of a K-step pair;
//  * the epilogue is conv3_pdma's (v_permlane16_swap -> 16-byte stores; the DPP row = the 16 pixels of a tile row).
struct CfgWS16 {
  static constexpr int HH = 18, HW = 18, NPIXP = HH * HW;
  static constexpr int PIECES = NPIXP * 8;
  static constexpr int NWAVE = 8;
  static constexpr int NINSTR = (PIECES + 63) / 64;             // 41
  static constexpr int NDMA = (NINSTR + NWAVE - 1) / NWAVE;     // 6 per wave per tile (surplus ones hit a dummy KiB)
  static constexpr int A_BYTES = NINSTR * 1024;
  static constexpr int NBUF = 3;
  static constexpr int DUMMY = NBUF * A_BYTES;
  static constexpr int RED_BASE = DUMMY + 1024;
  static constexpr int RED_BYTES = 2 * 2 * 4 * 64 * 4;          // [2 tiles][2 statistics][4 pixel-wave slots][64 channels]
  static constexpr int CT_BASE = RED_BASE + RED_BYTES;
  static constexpr int LDS = CT_BASE + 3 * 64 * 4;
  static constexpr int ROWS = 64;
};

template <bool ACC, int STATS = 0>
__global__ __launch_bounds__(512, 1) void conv3_ws16_kernel(const IgemmParams P, int tiles_per_block) {
  using C = CfgWS16;
  static_assert(!(ACC && STATS), "the gradient fan-in form carries no statistics");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef __attribute__((address_space(3))) void lds_void;
  constexpr unsigned OOB = 0xFFFFFFF0u;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wco = wave & 1, wpx = wave >> 1;
  const int l15 = lane & 15, kb = lane >> 4;
  const int nCg = P.Cout / C::ROWS;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int cg = slot % nCg, tr = (slot / nCg) * 8 + xcd;
  const int tiles_img = P.tilesX * P.tilesY;
  const int total_tiles = P.N * tiles_img;
  const int t_begin = tr * tiles_per_block;
  const int t_end = min(t_begin + tiles_per_block, total_tiles);
  if (t_begin >= t_end) {
    if (STATS && tid < 128)                       // an empty tile range still owns a partial: zeros
      P.stats[((size_t)tr * 2 + (tid >> 6)) * P.Cout + cg * C::ROWS + (tid & 63)] = 0.f;
    return;
  }
  float* const red = reinterpret_cast<float*>(smem + C::RED_BASE);
  float* const ctab = reinterpret_cast<float*>(smem + C::CT_BASE);      // [scale | shift | mean][64]
  if (STATS == 2 && tid < 192) {
    const float* srcp = tid < 64 ? P.bn_scale : (tid < 128 ? P.bn_shift : P.bn_mean);
    ctab[tid] = srcp[cg * C::ROWS + (tid & 63)];
  }
  float stat_tot = 0.f;
  const int ch0 = cg * C::ROWS + wco * 32;          // first output channel of this wave
  // (the gradient fan-in form keeps every wave's DMAs in front: its old-value loads are builtin loads, whose
  //  compiler-placed wait would drain DMAs issued behind them; the fused BatchNorm-backward form too: its y loads would
  //  need a vmcnt(0) in front of the late burst and the extra code path costs it 6 more spills -- measured 605 -> 828 us/step)
  const bool late = !ACC && STATS != 2 && __builtin_amdgcn_readfirstlane(wave) < 4;
  // ... and the other half (waves 4-7) keeps a tile's packed results in registers across the barrier and stores them at
  // the top of the NEXT tile, behind its DMA burst: every vector-memory instruction of a wave is then issued while its
  // SIMD partner runs MFMAs (a store or DMA that waits for a queue slot stalls the wave that issues it, and at the old
  // tile end both waves of a SIMD stalled together).
  const bool defer = !ACC && STATS != 2 && __builtin_amdgcn_readfirstlane(wave) >= 4;

  // ---- this wave's weights -> registers: A fragment (tile ct, tap, ks) = W[ch0 + 16ct + l15][tap][32ks + 8kb .. +7]
  bf16x8 wreg[2][18];
  {
    const bf16_t* wp = reinterpret_cast<const bf16_t*>(P.w);
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          wreg[ct][tap * 2 + ks] = *reinterpret_cast<const bf16x8*>(
              wp + ((size_t)(tap * P.Cout + ch0 + ct * 16 + l15)) * P.wK + ks * 32 + kb * 8);
    __builtin_amdgcn_s_waitcnt(0x0F70);          // retire the weight loads here (see conv3_ws_kernel)
  }

  // ---- pixel-fragment addresses: pixel p = (4 wpx + pt + r) * 18 + l15 + c of the patch, piece (4ks + kb) ^ (p & 7).
  // (p & 7) = (b + l15) & 7 with b = (2 (pt + r) + c) & 7 a compile-time constant of the read (72 wpx = 0 mod 8), so
  // vb[b] holds the lane part for K-step 0; K-step 1 flips bit 6; everything else is an immediate.  vb[] also carries
  // the byte offset of the ring slot being read and is stepped in place from tile to tile.
  unsigned vb[8];
#pragma unroll
  for (int b = 0; b < 8; ++b) vb[b] = (unsigned)((wpx * 4 * C::HW + l15) * 128 + ((kb ^ ((b + l15) & 7)) << 4));
  const DView S = P.src[0];
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  // DMA lane offsets relative to the patch origin (tile-invariant): lane q of instruction j fetches piece pos ^ (pp & 7)
  // of patch pixel pp = q >> 3 (beyond the patch: dropped).  The tile enters through the descriptor's base address
  // (scalar arithmetic), so an interior tile costs no vector instruction per DMA; a tile on the frame's edge checks its
  // halo pixels per lane.
  unsigned a_rel[C::NDMA];
#pragma unroll
  for (int j = 0; j < C::NDMA; ++j) {
    const int q = (j * C::NWAVE + wave) * 64 + lane;
    const int pp = q >> 3, pos = q & 7;
    const int hy = pp / C::HW, hx = pp - hy * C::HW;
    a_rel[j] = pp < C::NPIXP ? (unsigned)((hy * S.W + hx) * S.C * 2 + ((pos ^ (pp & 7)) << 4)) : OOB;
  }
  const unsigned img_bytes = (unsigned)S.H * S.W * S.C * 2u;

  struct TileIt { int n, ty, tx; };
  auto tile_at = [&](int tile) {
    TileIt it;
    it.n = tile / tiles_img;
    const int r = tile - it.n * tiles_img;
    it.ty = r / P.tilesX;
    it.tx = r - it.ty * P.tilesX;
    return it;
  };
  auto tile_next = [&](TileIt& it) {
    if (++it.tx == P.tilesX) {
      it.tx = 0;
      if (++it.ty == P.tilesY) { it.ty = 0; ++it.n; }
    }
  };
  TileIt dma_it = tile_at(t_begin), geo_it = dma_it;

  auto dma_a = [&](int buf, bool live) {         // the patch of the tile at dma_it (then advance); dead = to the dummy KiB
    const int ym1 = dma_it.ty * 16 - 1, xm1 = dma_it.tx * 16 - 1;
    // base = the patch origin (it may lie in front of the image: only lanes of pixels inside the frame carry an offset
    // below num_records; a valid lane's offset stays below 18 rows of the frame)
    const long long org = ((long long)ym1 * S.W + xm1) * (S.C * 2);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(S.p + (long long)(live ? dma_it.n : 0) * img_bytes + org), (short)0, 0x7FFFFFF0, 0x00020000);
    const bool inner = live && ym1 >= 0 && xm1 >= 0 && ym1 + C::HH <= S.H && xm1 + C::HW <= S.W;
    if (inner) {
#pragma unroll
      for (int j = 0; j < C::NDMA; ++j) {
        const int idx = j * C::NWAVE + wave_s;
        char* dst = idx < C::NINSTR ? smem + buf * C::A_BYTES + idx * 1024 : smem + C::DUMMY;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)dst, 16, a_rel[j], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int j = 0; j < C::NDMA; ++j) {
        int q = (j * C::NWAVE + wave_s) * 64 + lane;
        asm volatile("" : "+v"(q));                 // (per tile: hoisted out of the loop it costs live registers)
        const int pp = q >> 3;
        const int hy = pp / C::HW, hx = pp - hy * C::HW;
        const unsigned y = (unsigned)(ym1 + hy), x = (unsigned)(xm1 + hx);
        const bool ok = live && y < (unsigned)S.H && x < (unsigned)S.W;
        const unsigned vo = ok ? a_rel[j] : OOB;
        const int idx = j * C::NWAVE + wave_s;
        char* dst = (live && idx < C::NINSTR) ? smem + buf * C::A_BYTES + idx * 1024 : smem + C::DUMMY;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)dst, 16, vo, 0, 0, 0);
      }
    }
    tile_next(dma_it);
  };

  constexpr int NVIEW = STATS ? 1 : 2;           // the statistics forms write ONE dense destination
  constexpr int NST = 4 * NVIEW;                 // stores per wave per tile: 4 pixel rows x dst views
  constexpr int NY = STATS == 2 ? 4 : 0;         // y loads per tile (inline asm, hand-counted)
  static_assert(2 * NST + C::NDMA + NY <= 63, "vmcnt range");
  constexpr bool ALWAYS = STATS == 2;            // that form always issues its NDMA instructions: one wait form

  // Dense frames only (the launcher sends everything else to conv3_ws_kernel): whole 16x16 tiles, every destination view
  // covers the frame at offset 0.  A lane's offset inside a tile never changes (ovb: pixel row 0 of its four, per view;
  // rows 1-3 through the scalar offset operand, which the range check ignores: a lane that does not store carries an
  // out-of-range offset) and the tile enters through the descriptors' base addresses: scalar arithmetic only, where the
  // general lane geometry was ~200 vector instructions per tile.
  __amdgpu_buffer_rsrc_t drs[2];
  unsigned ovb[NVIEW];
  u32x4 pend[4];                                 // deferred stores: the packed results of the previous tile
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) pend[pt] = u32x4{0u, 0u, 0u, 0u};
  {
    const int co = ch0 + (kb & 1) * 16 + (kb >> 1) * 8;       // after the swap a lane holds 8 consecutive channels: tile (kb & 1), channels 8 (kb >> 1) .. + 7
#pragma unroll
    for (int q = 0; q < NVIEW; ++q) {
      const DViewW D = P.dst[q];
      const int cq = q == 0 ? co : co - P.dst_split;
      const bool mine = (q == 0) == (co < P.dst_split);
      ovb[q] = mine ? (unsigned)(((wpx * 4 * D.W + l15) * D.C + cq) * 2) : OOB;     // (an absent second view arrives as a copy of the first: no lane is its)
    }
  }
  // (tile 0's deferred group: NST stores against empty descriptors -- dropped, same vmcnt arithmetic)
#pragma unroll
  for (int q = 0; q < 2; ++q) drs[q] = __builtin_amdgcn_make_buffer_rsrc((void*)P.dst[0].p, (short)0, 0, 0x00020000);
  const unsigned rowb[2] = {(unsigned)(P.dst[0].W * P.dst[0].C * 2), (unsigned)(P.dst[1].W * P.dst[1].C * 2)};   // bytes per pixel row
  int n_img = 0;
  unsigned soff0 = 0;                            // byte offset of the tile in view 0 (the y loads add it too)
  auto geometry = [&]() {                        // of the tile at geo_it (then advance)
    const int n = geo_it.n;
    const int ty0 = geo_it.ty * 16, tx0 = geo_it.tx * 16;
    tile_next(geo_it);
    n_img = n;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const DViewW D = P.dst[q];
      const unsigned dimg = (unsigned)D.H * D.W * D.C * 2u;
      const unsigned so = (unsigned)((ty0 * D.W + tx0) * D.C * 2);
      if (q == 0) soff0 = so;
      drs[q] = __builtin_amdgcn_make_buffer_rsrc((void*)(D.p + (size_t)n * dimg + so), (short)0, (int)(dimg - so), 0x00020000);
    }
  };
  auto take_slots = [&](int kk) {                // the four pixel-wave slots of tile kk -> this thread's running total
    if (STATS && tid < 128) {
      const float* rp = red + (kk & 1) * 512 + (tid >> 6) * 256 + (tid & 63);
#pragma unroll
      for (int sl = 0; sl < 4; ++sl) stat_tot += rp[sl * 64];
    }
  };

#pragma unroll
  for (int d = 0; d < C::NBUF - 1; ++d)
    if (ALWAYS || t_begin + d < t_end) dma_a(d, t_begin + d < t_end);
  int cur = 0;
  // diagnostic build (stamps.h; nothing in the default build): per-wave cycle sums over all tiles.  Laps: 0 the counted
  // vmcnt wait, 1 the barrier, 2 the top of the tile (DMA / deferred stores / geometry), 3 the MFMA loop, 4 the late
  // DMA, 5 epilogue + stores.  Every stamp is fenced (mark<true>).
  StampClock clk;
  clk.start();
  for (int tile = t_begin; tile < t_end; ++tile) {
    const int k = tile - t_begin;
    const bool next_in_flight = ALWAYS || tile + 1 < t_end;
    // vmcnt counts loads, DMAs and stores in issue order: younger than tile k's patch are stores(k-2), y(k-1),
    // DMA(k+1), stores(k-1)  (see conv3_ws_kernel)
    if (k >= 2) {
      if (next_in_flight) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NST + C::NDMA + NY) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NST) : "memory");
    } else if (k == 1) {
      if (next_in_flight) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NST + C::NDMA + NY) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NST) : "memory");
    } else {
      if (next_in_flight) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NDMA) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    clk.mark<true>(0);
    __builtin_amdgcn_s_barrier();
    clk.mark<true>(1);
    if (k >= 1) take_slots(k - 1);
    constexpr bool RING2 = !ACC && STATS != 2;
    if constexpr (RING2) {
      // per-wave order of vector-memory operations in a tile: DMA(k + 2), then ONE group of NST stores -- tile k's own
      // at its end (waves 0-3 and the lock-step form) or tile k - 1's here (waves 4-7): the counted waits above hold for both
      if (!late) {
        if (tile + C::NBUF - 1 < t_end) dma_a((k + C::NBUF - 1) % C::NBUF, true);
      }
      if (defer) {
#pragma unroll
        for (int pt = 0; pt < 4; ++pt)
#pragma unroll
          for (int q = 0; q < NVIEW; ++q) __builtin_amdgcn_raw_buffer_store_b128(pend[pt], drs[q], ovb[q], pt * rowb[q], 0);
      }
    }
    geometry();
    const int n = n_img;
    (void)n;
    u32x4 yv[STATS == 2 ? 4 : 1];
    if constexpr (STATS == 2) {
      const unsigned dimg = (unsigned)P.dst[0].H * P.dst[0].W * P.dst[0].C * 2u;
      const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(P.bn_y + (size_t)n * dimg + soff0), (short)0, (int)(dimg - soff0), 0x00020000);
#pragma unroll
      for (int pt = 0; pt < 4; ++pt)             // inline asm + hand-counted wait (hipcc does not count LDS-DMAs)
        asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(yv[pt]) : "v"(ovb[0]), "s"(yrs), "s"(pt * rowb[0]) : "memory");
    }
    // The patch DMAs of tile k + 2.  A wave inside its burst of six one-KiB issues feeds no MFMAs, and with all eight
    // waves bursting behind the barrier the matrix pipe idles for the whole burst (r02 stamps: the burst costs as much
    // as the tile's 72 MFMAs).  The two waves of a SIMD (w, w + 4) therefore issue at opposite ends of the tile: waves
    // 4-7 here, waves 0-3 -- the older ones, which win the SIMD's issue arbitration and so should compute first -- behind
    // their MFMAs, still in front of the tile's stores (the vmcnt bookkeeping above counts the same operations either way).
    if constexpr (!RING2) {
      if (ALWAYS || tile + C::NBUF - 1 < t_end) dma_a((k + C::NBUF - 1) % C::NBUF, tile + C::NBUF - 1 < t_end);
    }
    u32x4 oldv[ACC ? 4 : 1];
    if constexpr (ACC) {                          // gradient fan-in: the old values, behind the tile's MFMAs
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) {
        const bool second = ovb[0] == OOB;
        const bool want = (P.accumulate >> (second ? 1 : 0)) & 1;
        const unsigned vo = want ? (second ? ovb[NVIEW - 1] : ovb[0]) : OOB;
        oldv[pt] = second ? __builtin_amdgcn_raw_buffer_load_b128(drs[1], vo, pt * rowb[1], 0)
                          : __builtin_amdgcn_raw_buffer_load_b128(drs[0], vo, pt * rowb[0], 0);
      }
    }

    clk.mark<true>(2);
    f32x4 acc[2][4];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) acc[ct][pt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // 18 K-steps (tap, 32-channel half) of 2 x 4 MFMAs; the four pixel fragments of step i + 1 are requested before the
    // MFMAs of step i and pinned there
    auto frag = [&](int i, int pt) {
      const int tap = i >> 1, ks = i & 1, r = tap / 3, c = tap % 3;
      const int b = (2 * (pt + r) + c) & 7;
      const unsigned a = (ks ? vb[b] ^ 64u : vb[b]);
      return *reinterpret_cast<const bf16x8*>(smem + a + ((pt + r) * C::HW + c) * 128);
    };
    // (the forms that hold y / old values across the loop have 16 registers fewer: ONE fragment set, each fragment
    //  re-requested for the next step right behind the two MFMAs that read it -- six MFMAs of cover)
    bf16x8 ring[RING2 ? 2 : 1][4];
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) ring[0][pt] = frag(0, pt);
#ifdef WS16_NO_MFMA           // diagnostic build: the tile's DMAs / stores / barriers without its MFMAs and fragment reads
    if (false)
#endif
#pragma unroll
    for (int i = 0; i < 18; ++i) {
      if constexpr (RING2) {
        if (i + 1 < 18) {
#pragma unroll
          for (int pt = 0; pt < 4; ++pt) ring[(i + 1) & 1][pt] = frag(i + 1, pt);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
          for (int pt = 0; pt < 4; ++pt)
            acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wreg[ct][i], ring[i & 1][pt], acc[ct][pt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      } else {
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) {
          __builtin_amdgcn_sched_barrier(0);
          acc[0][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wreg[0][i], ring[0][pt], acc[0][pt], 0, 0, 0);
          acc[1][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wreg[1][i], ring[0][pt], acc[1][pt], 0, 0, 0);
          if (i + 1 < 18) ring[0][pt] = frag(i + 1, pt);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    clk.mark<true>(3);
    // the ring slot of the next tile
    {
      const int nxt = (cur + 1) % C::NBUF;
      const unsigned delta = (unsigned)((nxt - cur) * C::A_BYTES);
#pragma unroll
      for (int b = 0; b < 8; ++b) vb[b] += delta;
      cur = nxt;
    }

    if constexpr (STATS == 2) {                   // the y loads are older than this tile's NDMA instructions ...
      if (late) asm volatile("s_waitcnt vmcnt(0)" : "+v"(yv[0]), "+v"(yv[1]), "+v"(yv[2]), "+v"(yv[3]));   // ... not issued yet
      else asm volatile("s_waitcnt vmcnt(%4)" : "+v"(yv[0]), "+v"(yv[1]), "+v"(yv[2]), "+v"(yv[3]) : "n"(C::NDMA));
    }
    if (late) {
      if (ALWAYS || tile + C::NBUF - 1 < t_end) dma_a((k + C::NBUF - 1) % C::NBUF, tile + C::NBUF - 1 < t_end);
    }

    clk.mark<true>(4);
    // ---- epilogue: D of 16x16x32: column = lane & 15 (pixel), rows 4 kb + j (channel of the 16-tile).  Exactly NST
    // buffer stores per wave (an OOB offset = dropped).
    float sa[4] = {0.f, 0.f, 0.f, 0.f}, sb[4] = {0.f, 0.f, 0.f, 0.f}, qa[4] = {0.f, 0.f, 0.f, 0.f}, qb[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      float va[4], vv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { va[j] = acc[0][pt][j]; vv[j] = acc[1][pt][j]; }
      bf16x4 ra, rb;
      if constexpr (ACC) {
        const u32x4 o = oldv[pt];                  // stored layout -> the accumulator's (the exchange is an involution)
        const auto o0 = __builtin_amdgcn_permlane16_swap(o[0], o[2], false, false);
        const auto o1 = __builtin_amdgcn_permlane16_swap(o[1], o[3], false, false);
        const bf16x4 oa = __builtin_bit_cast(bf16x4, u32x2{o0[0], o1[0]});
        const bf16x4 ob = __builtin_bit_cast(bf16x4, u32x2{o0[1], o1[1]});
#pragma unroll
        for (int j = 0; j < 4; ++j) { ra[j] = (bf16_t)(va[j] + (float)oa[j]); rb[j] = (bf16_t)(vv[j] + (float)ob[j]); }
      } else if constexpr (STATS == 2) {
        const u32x4 o = yv[pt];
        const auto o0 = __builtin_amdgcn_permlane16_swap(o[0], o[2], false, false);
        const auto o1 = __builtin_amdgcn_permlane16_swap(o[1], o[3], false, false);
        const bf16x4 ya = __builtin_bit_cast(bf16x4, u32x2{o0[0], o1[0]});
        const bf16x4 yb = __builtin_bit_cast(bf16x4, u32x2{o0[1], o1[1]});
        // (dense frames: every tile pixel is a frame pixel.)  The 3 x 4 coefficients of a channel half are re-read from
        // LDS per pixel row and half -- 12 live registers instead of 24 in a kernel that must not spill: scratch traffic
        // inside the loop would join the hand-counted vmcnt stream
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          asm volatile("" ::: "memory");
          const int cb = wco * 32 + 16 * t + 4 * kb;
          const f32x4 sc = *reinterpret_cast<const f32x4*>(ctab + cb);
          const f32x4 sh = *reinterpret_cast<const f32x4*>(ctab + 64 + cb);
          const f32x4 mu = *reinterpret_cast<const f32x4*>(ctab + 128 + cb);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float fy = (float)(t ? yb[j] : ya[j]);
            const bf16_t r = (bf16_t)(fmaf(fy, sc[j], sh[j]) > 0.f ? (t ? vv[j] : va[j]) : 0.f);
            const float q0 = (float)r;                                         // dz as stored
            if (t) { rb[j] = r; sb[j] += q0; qb[j] = fmaf(q0, fy - mu[j], qb[j]); }
            else { ra[j] = r; sa[j] += q0; qa[j] = fmaf(q0, fy - mu[j], qa[j]); }
          }
        }
      } else {
        if (P.bias) {                              // inference: BatchNorm shift (+ ReLU) of the folded layer
          const float* bp = P.bias + ch0 + kb * 4;
#pragma unroll
          for (int j = 0; j < 4; ++j) { va[j] += bp[j]; vv[j] += bp[16 + j]; }
        }
        if (P.relu) {
#pragma unroll
          for (int j = 0; j < 4; ++j) { va[j] = fmaxf(va[j], 0.f); vv[j] = fmaxf(vv[j], 0.f); }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { ra[j] = (bf16_t)va[j]; rb[j] = (bf16_t)vv[j]; }
        if constexpr (STATS == 1) {
          constexpr bool ok = true;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float q0 = ok ? (float)ra[j] : 0.f, q1 = ok ? (float)rb[j] : 0.f;   // the values as stored
            sa[j] += q0; qa[j] = fmaf(q0, q0, qa[j]);
            sb[j] += q1; qb[j] = fmaf(q1, q1, qb[j]);
          }
        }
      }
      const u32x2 ua = __builtin_bit_cast(u32x2, ra), ub = __builtin_bit_cast(u32x2, rb);
      const auto s0 = __builtin_amdgcn_permlane16_swap(ua[0], ub[0], false, false);
      const auto s1 = __builtin_amdgcn_permlane16_swap(ua[1], ub[1], false, false);
      const u32x4 bits = u32x4{s0[0], s1[0], s0[1], s1[1]};
      pend[pt] = bits;             // (unconditional: dead across the MFMA loop for the register allocator)
      if (!defer) {
#pragma unroll
        for (int q = 0; q < NVIEW; ++q) {
#ifdef WS16_NO_STORE          // diagnostic build: every store dropped (out-of-range offset), counts unchanged
          __builtin_amdgcn_raw_buffer_store_b128(bits, drs[q], OOB, 0, 0);
#else
          __builtin_amdgcn_raw_buffer_store_b128(bits, drs[q], ovb[q], pt * rowb[q], 0);
#endif
        }
      }
    }
    if constexpr (STATS != 0) {
      // the DPP row is the 16 pixels of a tile row: one reduction leaves a (statistic, channel) total of this wave's
      // 64 pixels in every lane; the four row leaders (l15 == 0, one per kb) file them in this pixel-wave's slot
      float rv[16];
#pragma unroll
      for (int j = 0; j < 4; ++j) { rv[j] = sa[j]; rv[4 + j] = sb[j]; rv[8 + j] = qa[j]; rv[12 + j] = qb[j]; }
      row16_sum_n(rv);
      if (l15 == 0) {
        float* rw = red + (k & 1) * 512 + wpx * 64 + wco * 32 + 4 * kb;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          rw[j] = rv[j]; rw[16 + j] = rv[4 + j];
          rw[256 + j] = rv[8 + j]; rw[256 + 16 + j] = rv[12 + j];
        }
      }
    }
    clk.mark<true>(5);
  }
  // (the masked-gradient form stays unstamped: it has no registers for the sums -- with the write-out the diagnostic
  //  build spills 44 bytes to scratch, and scratch traffic joins the hand-counted vmcnt stream)
  if (STATS != 2) clk.store(STAMP_SINK(P.stamps), 8, (unsigned long long)(t_end - t_begin));
  if (defer) {                                   // the last tile's results
#pragma unroll
    for (int pt = 0; pt < 4; ++pt)
#pragma unroll
      for (int q = 0; q < NVIEW; ++q) __builtin_amdgcn_raw_buffer_store_b128(pend[pt], drs[q], ovb[q], pt * rowb[q], 0);
  }
  if constexpr (STATS != 0) {
    // the last tile's slots, then ONE partial per block.  (The thread index is re-derived here: values computed from the
    // launch-time one before the loop would be spilled across it, and scratch traffic joins the hand-counted vmcnt stream.)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const int tid2 = wave_s * 64 + (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    if (tid2 < 128) {
      const float* rp = red + ((t_end - 1 - t_begin) & 1) * 512 + (tid2 >> 6) * 256 + (tid2 & 63);
#pragma unroll
      for (int sl = 0; sl < 4; ++sl) stat_tot += rp[sl * 64];
      P.stats[((size_t)tr * 2 + (tid2 >> 6)) * P.Cout + cg * C::ROWS + (tid2 & 63)] = stat_tot;
    }
  }
  if constexpr (ALWAYS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // drain the dummy DMAs before the wave ends
}

}  // namespace

int32_t unet_internal_conv3_ws(IgemmParams P, int kclass, hipStream_t s, int* stat_parts) {
  using C = CfgWS;
  const bool stats_ok = !P.accumulate && P.dst_split == P.Cout && covers_frame(P.dst[0], P);
  const int mode = P.bn_y ? 2 : ((P.stats && stats_ok) ? 1 : 0);
  UNET_REQUIRE(mode != 2 || stats_ok, UNET_ERR_UNSUPPORTED, "conv3_ws: fused BatchNorm backward needs one dense destination");
  // dense 16-aligned frames: the 16x16x32 kernel (conv3_ws16_kernel; every form of it is spill-free --
  // tools/check_dpp_hazards.py asserts that; 18.87 -> 18.71 ms per step when it came in)
  bool dense16 = P.H % 16 == 0 && P.W % 16 == 0;
  for (int q = 0; q < 2; ++q)
    if (P.dst[q].p && !covers_frame(P.dst[q], P)) dense16 = false;
  void (*kern)(const IgemmParams, int);
  int tile_h, tile_w, rows, lds_bytes;
  double alg_bytes = 0.0;                         // (conv3_ws_kernel's bracket states none)
  const char* what;
  if (dense16) {
    if (!P.dst[1].p) P.dst[1] = P.dst[0];         // no lane stores to it (dst_split == Cout); saves the kernel a select per tile
    kern = P.accumulate ? conv3_ws16_kernel<true, 0>
                        : (mode == 2 ? conv3_ws16_kernel<false, 2> : (mode == 1 ? conv3_ws16_kernel<false, 1> : conv3_ws16_kernel<false, 0>));
    tile_h = tile_w = 16;  rows = CfgWS16::ROWS;  lds_bytes = CfgWS16::LDS;  what = "conv3_ws16_kernel";
    unet_set_max_lds(reinterpret_cast<const void*>(kern), lds_bytes);
    const double px = (double)P.N * P.H * P.W;
    alg_bytes = 2.0 * (px * (P.Ctot + P.Cout * (1.0 + (mode == 2 ? 1 : 0) + (P.accumulate ? 1 : 0))) + 9.0 * P.Ctot * P.Cout);
#ifdef PDMA_STAMPS
    P.stamps = g_stamp_sink;
#endif
  } else {                // (ragged frames / offset views: conv3_ws_kernel's per-lane geometry)
    kern = P.accumulate ? conv3_ws_kernel<true, 0>
                        : (mode == 2 ? conv3_ws_kernel<false, 2> : (mode == 1 ? conv3_ws_kernel<false, 1> : conv3_ws_kernel<false, 0>));
    tile_h = C::WTH;  tile_w = C::WTW;  rows = C::ROWS;  lds_bytes = C::LDS;  what = "conv3_ws_kernel";
  }
  P.tilesX = cdiv(P.W, tile_w);
  P.tilesY = cdiv(P.H, tile_h);
  const long long tiles = (long long)P.N * P.tilesY * P.tilesX;
  const int nCg = P.Cout / rows;
  int tpb = (int)cdiv64(tiles * nCg, unet_cu_budget());        // one resident block per CU, one round
  if (tpb < 2) tpb = 2;
  const long long ranges8 = cdiv64(cdiv64(tiles, tpb), 8) * 8;      // tile ranges, padded to a multiple of 8 (XCDs)
  const long long blocks = ranges8 * nCg;
  const double flops = 2.0 * P.N * P.H * P.W * (double)P.Cout * P.Ctot * 9;
  if (mode == 0) P.stats = nullptr;               // (statistics, if wanted, by the caller's streaming pass)
  if (stat_parts) *stat_parts = mode ? (int)ranges8 : 0;          // one ordered partial per tile range
  ProfScope prof(kclass, flops, s, mode == 2 ? "conv3_ws_bnbwd_kernel" : "conv3_ws_kernel", alg_bytes);
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(512), lds_bytes, s, P, tpb);
  return unet_check_launch(what);
}
