// conv3_pdma_kernel<BN>: the 3x3 convolution (forward and data gradient) of every 16-aligned bf16 layer with at least
// 128 input channels, BOTH operands staged by LDS-DMA, persistent blocks.
//   One 512-thread block per CU owns 16x16 output pixels x BN (128 or 64) output channels at a time (8 waves x
//   (BN/2 co x 64 px) on v_mfma_f32_16x16x32_bf16).  Compared with conv3m16_kernel (two 256-thread blocks per CU,
//   each staging its own weight slab through registers + ds_write_b128) the weight slab of a tap is fetched ONCE per
//   CU and written to LDS by the DMA engine: half the L2 traffic per MFMA and no ds_write_b128 (79 B/clk) competing
//   with the fragment reads for the LDS array, which is what held the old kernel at 46 % MFMA busy.
//   LDS: two halo'd 18x18 pixel patches of one 64-channel chunk (rows padded to 160 B: conflict-free 16x16x32
//   fragments) + a 3-slot ring of BN x 64 weight slabs (unpadded 128-B rows, 16-B pieces XOR-swizzled by
//   (row>>1)&7 through the DMA's per-lane SOURCE address).  Weight slabs are issued two taps ahead, the next
//   chunk's patch is issued one DMA per wave per tap during the current chunk; every wait is a counted vmcnt.
//   PERSISTENT: a block walks a list of (output-channel tile, pixel tile) work items; the DMA stream (patch of the
//   next chunk, weight slabs two taps ahead) simply continues into the next work item, so a block's un-overlapped
//   prologue is paid once per launch instead of once per tile, and the epilogue's stores drain behind the next
//   tile's MFMAs.  That is what the 128-input-channel layers (2 chunks = 18 steps per tile) needed.
// Work order: consecutive work items = consecutive pixel tiles of ONE channel tile, and XCD x owns a contiguous
// run of them, so the blocks of an XCD stream the same weight slabs and neighbouring halos through its L2.
#include "conv_common.h"

namespace {

// Work order of conv3_pdma: item wk -> (channel tile, pixel tile).  XCD x owns 32 consecutive items per round; with
// co_il = c those are 32 / c pixel tiles x c channel tiles (super-groups of c channel tiles are walked tile-major), so the
// c blocks that read the SAME input patches run on one L2 at the same time and the patch leaves the Infinity Cache / HBM
// once per super-group instead of once per channel tile (c = 1: channel-tile-major, every channel tile re-streams X).
__device__ __forceinline__ void pdma_item(int wk, int n_tiles, int c, int& cot, int& tile) {
  const int span = c * n_tiles;
  const int sg = wk / span, rem = wk - sg * span;
  tile = rem / c;
  cot = sg * c + (rem - tile * c);
}

template <int BN, bool PAIR = false>
struct CfgP {
  static constexpr int TH = 16, TW = 16, HH = 18, HW = 18;
  static constexpr int PSTR = 160, PPP = 10, RS = HW * PSTR;
  static constexpr int A_INSTR = (HH * HW * PPP + 63) / 64;         // 51 wave-instructions of 1 KiB
  static constexpr int A_BYTES = A_INSTR * 1024;
  static constexpr int NDA = (A_INSTR + 7) / 8;                      // 7 per wave
  // PAIR (BN = 64): a ring slot holds the slabs of TWO consecutive taps (a step = two taps between barriers)
  static constexpr int W_BYTES = (PAIR ? 2 : 1) * BN * 128, NDW = W_BYTES / 1024 / 8; // 2 (BN 128, PAIR) or 1 (BN 64) per wave
  static constexpr int NSLOT = 3;
  // the weight ring sits FIRST: slot * W_BYTES (<= 32 KiB) then folds into the 16-bit offset field of the fragment
  // ds_reads (behind the patches, at 102 KiB, every read cost a v_add and the tap a spilled-SGPR v_readlane)
  static constexpr int W_BASE = 0;
  static constexpr int A_BASE = NSLOT * W_BYTES;
  static constexpr int RED_BASE = A_BASE + 2 * A_BYTES;              // BatchNorm partials of the epilogue
  static constexpr int RED_BYTES = 4 * 2 * BN * 4;
  static constexpr int DUMMY = RED_BASE + RED_BYTES;
  static constexpr int LDS = DUMMY + 1024;
  static constexpr int CT = BN / 32;                                 // 16-channel MFMA tiles per wave (2 waves along channels)
  static constexpr int NST = CT / 2 * 4;                             // 16-byte output stores per lane per work item
};

// PP ("ping-pong"): the two waves of a SIMD (w, w + 4) run HALF A STEP apart.  Waves 0-3 own the tile's first BN/2
// output channels, waves 4-7 the second; a step is [LOAD: 16 fragment reads of the tap, this wave's LDS-DMA issues, the
// counted vmcnt, lgkmcnt(0)] s_barrier [COMPUTE: the tap's 32 MFMAs straight from registers] s_barrier, and waves 4-7
// start one barrier late -- while one wave of a SIMD feeds the matrix pipe its partner reads LDS and issues DMAs,
// instead of all eight bursting their DMAs and fragment reads together behind one barrier per tap (stamps: 35-45 % of a
// lock-step tap went to the DMA issue burst, profiles/r02_pdma_stamps.txt).  LDS hazards at distance one barrier: a
// slab / patch buffer is re-filled by DMAs issued in the slot after its last reads, which are retired (lgkmcnt(0))
// BEFORE the barrier that ends their LOAD.
// PAIR (round 4; BN = 64, exactly two 64-channel chunks = the 128 -> 64 layers at 256 x 256 and the 128 -> 64 data
// gradient): with 64-channel tiles a tap is only 16 MFMAs per wave, and the stamps (profiles/r04_pdma64_stamps.txt) put
// ~800 of its 1 300 cycles into what a tap costs regardless of its size -- the barrier skew, the DMA-issue burst, the
// fragment-read latency in front of the first MFMA.  A STEP is therefore two consecutive taps of the 18 of a work item
// (9 steps; step 4 straddles the chunks): one barrier, one counted wait and one DMA burst per 32 MFMAs, as in the
// 128-channel kernel; a ring slot holds both taps' weight slabs (16 KiB, the 128-channel ring), the second tap's
// fragments are fetched behind the first tap's MFMAs.  Same accumulation order, bit-identical outputs.
template <int BN, bool BNBWD = false, bool PP = false, bool PAIR = false>
__device__ __forceinline__ void conv3_pdma_body(const IgemmParams& P) {
  static_assert(!PAIR || (BN == 64 && !PP), "pair steps: the lock-step 64-channel kernel");
  using C = CfgP<BN, PAIR>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef __attribute__((address_space(3))) void lds_void;
  constexpr unsigned OOB = 0xFFFFFFF0u;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = wave >> 2;                     // PP: 0 = the leading half, 1 = one barrier behind
  const int wco = PP ? grp : (wave & 1), wpx = PP ? (wave & 3) : (wave >> 1);
  const int l15 = lane & 15, kb = lane >> 4;

  const int G = gridDim.x;                       // launch_pdma makes it a multiple of 8
  const int tiles_img = P.tilesY * P.tilesX;
  const int n_tiles = P.N * tiles_img;
  const int total = n_tiles * P.nCo;
  // XCD x (= blockIdx % 8) owns the contiguous logical range [x*G/8, (x+1)*G/8)
  const int logical = (blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3);
  if (logical >= total) return;

  int aoff[C::CT][2], boff[4];
#pragma unroll
  for (int ct = 0; ct < C::CT; ++ct) {
    const int row = wco * (BN / 2) + ct * 16 + l15;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) aoff[ct][ks] = row * 128 + (((ks * 4 + kb) ^ ((row >> 1) & 7)) << 4);
  }
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) boff[pt] = (wpx * 4 + pt) * C::RS + l15 * C::PSTR + kb * 16;

  // lane geometry of this wave's patch DMA pieces (constant), per-work offsets (a_g) derived from it
  int a_code[C::NDA];                            // hy | hx << 8 | part << 16, -1 = pad piece
#pragma unroll
  for (int j = 0; j < C::NDA; ++j) {
    const int q = (j * 8 + wave) * 64 + lane;
    const int pix = q / C::PPP, part = q - pix * C::PPP;
    const int hy = pix / C::HW, hx = pix - hy * C::HW;
    // bits 24-27: the pixel lies in the patch's top / bottom row, left / right column (the halo of a frame-edge tile)
    const int edge = (hy == 0) | ((hy == C::HH - 1) << 1) | ((hx == 0) << 2) | ((hx == C::HW - 1) << 3);
    a_code[j] = (pix < C::HH * C::HW && part < 8) ? (hy | (hx << 8) | (part << 16) | (edge << 24)) : -1;
  }
  unsigned w_g[C::NDW];                          // (PAIR: both instructions of a step use w_g[0], rows 0-63 of a tap's slab)
#pragma unroll
  for (int j = 0; j < C::NDW; ++j) {
    const int q = (j * 8 + wave) * 64 + lane;
    const int row = q >> 3, pos = q & 7;
    w_g[j] = (unsigned)((row * P.wK) * 2 + ((pos ^ ((row >> 1) & 7)) << 4));
  }

  const int nchunks = P.Ctot / 64;
  const unsigned w_tap_stride = (unsigned)P.Cout * P.wK * 2;
  const __amdgpu_buffer_rsrc_t w_rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)P.w, (short)0, (int)(9u * w_tap_stride), 0x00020000);
  const unsigned img0 = (unsigned)P.src[0].H * P.src[0].W * P.src[0].C * 2;
  const unsigned img1 = (unsigned)P.src[1].H * P.src[1].W * P.src[1].C * 2;

  // ---- DMA-side state: the work item whose patches / weights are being fetched
  unsigned a_g[2][C::NDA];
  __amdgpu_buffer_rsrc_t a_rsrc[2];
  unsigned d_wbase = 0;                          // byte offset of the work item's first weight row
  bool d_live = true;
  // Dense sources (P.pdma_dense_src: both views frame-sized at offset 0, one channel stride): a lane's patch offsets
  // relative to the patch origin never change -- kept in a_g[1][], which the general path uses for the second view -- and
  // the work item enters through the descriptors' base addresses; per item only the halo of a frame-edge tile is masked
  // (3 vector instructions per piece instead of ~17 x 2 views, in the last chunk's taps where issue slots are scarce).
  const bool dsrc = P.pdma_dense_src != 0;
  if (dsrc) {
#pragma unroll
    for (int j = 0; j < C::NDA; ++j) {
      const int code = a_code[j];
      const int hy = code & 255, hx = (code >> 8) & 255, part = (code >> 16) & 255;
      a_g[1][j] = code >= 0 ? (unsigned)(((hy * P.src[0].W + hx) * P.src[0].C) * 2 + part * 16) : OOB;
    }
  }
  auto setup_dma = [&](int wk) {
    int cot, tile;
    pdma_item(wk, n_tiles, P.co_il, cot, tile);
    const int n = tile / tiles_img, r = tile - n * tiles_img;
    const int ty0 = (r / P.tilesX) * C::TH, tx0 = (r % P.tilesX) * C::TW;
    d_wbase = (unsigned)(cot * BN) * P.wK * 2;
    if (dsrc) {
      const unsigned E = (unsigned)((ty0 == 0) | ((ty0 + C::TH == P.H) << 1) | ((tx0 == 0) << 2) | ((tx0 + C::TW == P.W) << 3)) << 24;
      // (the patch origin of a top / left tile lies in front of the image: only in-frame lanes carry an in-range offset)
      const long long tb = ((long long)(ty0 - 1) * P.src[0].W + (tx0 - 1)) * (P.src[0].C * 2);
      a_rsrc[0] = __builtin_amdgcn_make_buffer_rsrc((void*)(P.src[0].p + (long long)n * img0 + tb), (short)0, 0x7FFFFFF0, 0x00020000);
      a_rsrc[1] = __builtin_amdgcn_make_buffer_rsrc((void*)(P.src[1].p ? P.src[1].p + (long long)n * img1 + tb : P.src[0].p),
                                                    (short)0, P.src[1].p ? 0x7FFFFFF0 : 0, 0x00020000);
#pragma unroll
      for (int j = 0; j < C::NDA; ++j) a_g[0][j] = ((unsigned)a_code[j] & E) ? OOB : a_g[1][j];
      return;
    }
    a_rsrc[0] = __builtin_amdgcn_make_buffer_rsrc((void*)(P.src[0].p + (size_t)n * img0), (short)0, (int)img0, 0x00020000);
    a_rsrc[1] = __builtin_amdgcn_make_buffer_rsrc((void*)(P.src[1].p ? P.src[1].p + (size_t)n * img1 : P.src[0].p),
                                                  (short)0, P.src[1].p ? (int)img1 : 0, 0x00020000);
#pragma unroll
    for (int j = 0; j < C::NDA; ++j) {
      const int code = a_code[j];
      const int hy = code & 255, hx = (code >> 8) & 255, part = (code >> 16) & 255;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const DView S = P.src[k];
        const int y = ty0 + hy - 1 - S.oy, x = tx0 + hx - 1 - S.ox;
        a_g[k][j] = (code >= 0 && S.C > 0 && y >= 0 && y < S.H && x >= 0 && x < S.W)
                        ? (unsigned)(((y * S.W + x) * S.C) * 2 + part * 16) : OOB;
      }
    }
  };
  // wave-instruction j of the patch of `chunk` (of the DMA-side work item) into patch buffer `buf`
  auto dma_patch = [&](int chunk, int j, int buf, bool live) {
    const int idx = j * 8 + wave;
    live = live && idx < C::A_INSTR;
    char* dst = live ? smem + C::A_BASE + buf * C::A_BYTES + idx * 1024 : smem + C::DUMMY;
    const int ch = chunk * 64;
    if (ch < P.src[0].C) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rsrc[0], (lds_void*)dst, 16, live ? a_g[0][j] : OOB,
                                               (unsigned)ch * 2, 0, 0);
    } else {
      // (the two candidates pass through an opaque copy: folded into a load through a selected POINTER they would take the
      //  whole a_g array out of registers -- scratch traffic inside the hand-counted vmcnt stream)
      unsigned o0 = a_g[0][j], o1 = a_g[1][j];
      asm volatile("" : "+v"(o0), "+v"(o1));
      __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rsrc[1], (lds_void*)dst, 16, live ? (dsrc ? o0 : o1) : OOB,
                                               (unsigned)(ch - P.src[0].C) * 2, 0, 0);
    }
  };
  auto dma_w = [&](unsigned wbase, int chunk, int tap, int slot, bool live) {
    const unsigned soff = live ? wbase + (unsigned)tap * w_tap_stride + (unsigned)chunk * 128 : 0u;
#pragma unroll
    for (int j = 0; j < C::NDW; ++j) {
      char* dst = live ? smem + C::W_BASE + slot * C::W_BYTES + (j * 8 + wave) * 1024 : smem + C::DUMMY;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, (lds_void*)dst, 16, live ? w_g[j] : OOB, soff, 0, 0);
    }
  };

  // PAIR: the slabs of linear tap-steps (sA, sA + 1) of the work item whose first weight row is `wbase` into ring slot `slot`
  // (rows 0-63: tap A, rows 64-127: tap B; the same per-lane row / piece offsets, two scalar bases)
  auto dma_w2 = [&](unsigned wbase, int sA, int slot, bool live) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int sj = sA + j, cj = sj / 9, tj = sj - cj * 9;
      const unsigned soff = live ? wbase + (unsigned)tj * w_tap_stride + (unsigned)cj * 128 : 0u;
      char* dst = live ? smem + C::W_BASE + slot * C::W_BYTES + j * (BN * 128) + wave * 1024 : smem + C::DUMMY;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, (lds_void*)dst, 16, live ? w_g[0] : OOB, soff, 0, 0);
    }
  };

  f32x4 acc[C::CT][4];
  // One tap = two 32-channel half-steps (ks) of CT x 4 MFMAs.  The fragment reads are software-pipelined BY HAND and
  // pinned with sched_barriers: left alone, hipcc funnels the weight fragments through one register quad and waits
  // for each ds_read right before its MFMAs (eight exposed LDS latencies per tap; SQ_WAIT_ANY 44 %).  Here every
  // fragment is requested at least four MFMAs before its first use; at most 11 fragments are live.
  auto compute = [&](int pbuf, int toff, int slot) {
    const char* pa = smem + C::W_BASE + slot * C::W_BYTES;
    const char* pb = smem + pbuf + toff;
    auto ra = [&](int ks, int ct) { return *reinterpret_cast<const bf16x8*>(pa + aoff[ct][ks]); };
    auto rb = [&](int ks, int pt) { return *reinterpret_cast<const bf16x8*>(pb + boff[pt] + ks * 64); };
    auto mm = [&](int ct, const bf16x8& fa, const bf16x8 (&fb)[4]) {
#pragma unroll
      for (int pt = 0; pt < 4; ++pt)
        acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb[pt], acc[ct][pt], 0, 0, 0);
    };
    bf16x8 fb0[4], fb1[4];
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) fb0[pt] = rb(0, pt);
    if constexpr (C::CT == 4) {
      bf16x8 a0 = ra(0, 0), a1 = ra(0, 1);
      __builtin_amdgcn_sched_barrier(0);
      bf16x8 a2 = ra(0, 2), a3 = ra(0, 3);
      mm(0, a0, fb0);
      __builtin_amdgcn_sched_barrier(0);
      fb1[0] = rb(1, 0); fb1[1] = rb(1, 1);
      mm(1, a1, fb0);
      __builtin_amdgcn_sched_barrier(0);
      fb1[2] = rb(1, 2); fb1[3] = rb(1, 3);
      mm(2, a2, fb0);
      __builtin_amdgcn_sched_barrier(0);
      a0 = ra(1, 0); a1 = ra(1, 1);
      mm(3, a3, fb0);
      __builtin_amdgcn_sched_barrier(0);
      a2 = ra(1, 2);
      mm(0, a0, fb1);
      __builtin_amdgcn_sched_barrier(0);
      a3 = ra(1, 3);
      mm(1, a1, fb1);
      __builtin_amdgcn_sched_barrier(0);
      mm(2, a2, fb1);
      mm(3, a3, fb1);
    } else {
      // 8 MFMAs per half-step cannot cover an LDS round trip: the whole second half-step is fetched behind the first
      bf16x8 a0 = ra(0, 0), a1 = ra(0, 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) fb1[pt] = rb(1, pt);
      const bf16x8 a2 = ra(1, 0), a3 = ra(1, 1);
      mm(0, a0, fb0);
      mm(1, a1, fb0);
      __builtin_amdgcn_sched_barrier(0);
      mm(0, a2, fb1);
      mm(1, a3, fb1);
    }
  };

  // PAIR: two taps back to back (A then B: the accumulation order of two single taps); tap B's fragments are requested
  // behind tap A's MFMAs, so only the first half-step of a step waits for LDS
  auto compute2 = [&](int pbufA, int toffA, int pbufB, int toffB, int slot) {
    const char* pa = smem + C::W_BASE + slot * C::W_BYTES;
    const char* pbA = smem + pbufA + toffA;
    const char* pbB = smem + pbufB + toffB;
    auto ra = [&](int tb, int ks, int ct) { return *reinterpret_cast<const bf16x8*>(pa + tb * (BN * 128) + aoff[ct][ks]); };
    auto rb = [&](const char* pb, int ks, int pt) { return *reinterpret_cast<const bf16x8*>(pb + boff[pt] + ks * 64); };
    auto mm = [&](int ct, const bf16x8& fa_, const bf16x8 (&fb_)[4]) {
#pragma unroll
      for (int pt = 0; pt < 4; ++pt)
        acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa_, fb_[pt], acc[ct][pt], 0, 0, 0);
    };
    bf16x8 f0[4], f1[4], g0[4], g1[4];
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) f0[pt] = rb(pbA, 0, pt);
    const bf16x8 a0 = ra(0, 0, 0), a1 = ra(0, 0, 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) f1[pt] = rb(pbA, 1, pt);
    const bf16x8 a2 = ra(0, 1, 0), a3 = ra(0, 1, 1);
    mm(0, a0, f0);
    mm(1, a1, f0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) g0[pt] = rb(pbB, 0, pt);
    const bf16x8 c0 = ra(1, 0, 0), c1 = ra(1, 0, 1);
    mm(0, a2, f1);
    mm(1, a3, f1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) g1[pt] = rb(pbB, 1, pt);
    const bf16x8 c2 = ra(1, 1, 0), c3 = ra(1, 1, 1);
    mm(0, c0, g0);
    mm(1, c1, g0);
    __builtin_amdgcn_sched_barrier(0);
    mm(0, c2, g1);
    mm(1, c3, g1);
  };

  // PP: the same tap as two halves -- every fragment of the tap into registers, then nothing but MFMAs
  bf16x8 fa[2][C::CT], fb[2][4];
  auto load_frags = [&](int pbuf, int toff, int slot) {
    const char* pa = smem + C::W_BASE + slot * C::W_BYTES;
    const char* pb = smem + pbuf + toff;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) fb[ks][pt] = *reinterpret_cast<const bf16x8*>(pb + boff[pt] + ks * 64);
#pragma unroll
      for (int ct = 0; ct < C::CT; ++ct) fa[ks][ct] = *reinterpret_cast<const bf16x8*>(pa + aoff[ct][ks]);
    }
  };
  auto mma_frags = [&]() {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int ct = 0; ct < C::CT; ++ct)
#pragma unroll
        for (int pt = 0; pt < 4; ++pt)
          acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[ks][ct], fb[ks][pt], acc[ct][pt], 0, 0, 0);
  };

  // prologue: patch of chunk 0 and the first two weight slabs of the first work item
  setup_dma(logical);
#pragma unroll
  for (int j = 0; j < C::NDA; ++j) dma_patch(0, j, 0, true);
  if constexpr (PAIR) {
    dma_w2(d_wbase, 0, 0, true);
    dma_w2(d_wbase, 2, 1, true);
  } else {
    dma_w(d_wbase, 0, 0, 0, true);
    dma_w(d_wbase, 0, 1, 1, true);
  }
  if constexpr (PP) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NDW) : "memory");      // patch 0 + W(0) landed; W(1) in flight
    __builtin_amdgcn_s_barrier();
    if (grp) __builtin_amdgcn_s_barrier();                              // the stagger: waves 4-7 one barrier behind
  }

  // diagnostic build (stamps.h; nothing in the default build): per-wave cycle sums over all taps.  Lock-step laps: 0 the
  // counted vmcnt wait, 1 the barrier, 2 DMA issue, 3 fragment reads + MFMAs, 4 the epilogues.  Ping-pong laps: 0 fragment
  // reads + DMA issue (4: the reads' issue alone, inside 0), 1 the waits, 2 the barrier that ends LOAD, 3 MFMAs, 5 the
  // barrier that ends COMPUTE.  The clock is paused across an epilogue.
  StampClock clk;
  clk.start(false);
  int pbuf_i = 0;                                 // patch buffer of the chunk being computed
  bool after_epilogue = false;
  const bool late_dma = !PP && P.pdma_stagger && __builtin_amdgcn_readfirstlane(wave) < 4;
  // BatchNorm partial sums of this lane's outputs (4 channels x CT tiles, 2 statistics).  Block mode (P.zdiv: every
  // block visits every channel tile): a layer of thousands of tiles has 256 partials to finalise -- the block keeps a
  // running total per (statistic, channel) over its work items of one channel tile.  BN = 64 (DEFER): the per-lane sums
  // themselves run on across those items and are reduced over lanes and waves ONCE, at the last of them (the 64 DPP adds
  // + LDS exchange + barrier leave the per-item epilogue: +3 %).  At BN = 128 that is 32 more live registers: the lock-step
  // forward kernel has them since the output addressing went scalar (215 -> 247 VGPRs, +0..4 % per layer,
  // profiles/r03_pdma_dense_epilogue.txt); the ping-pong and BatchNorm-backward instantiations (251 / 236) would spill, so
  // there every item reduces and a thread carries the total.  Fixed order either way: deterministic.
  constexpr bool DEFER = BN == 64 || (!PP && !BNBWD);
  // Output addressing of dense destinations (P.pdma_dense: every destination view covers the frame at offset 0; frames are
  // whole 16x16 tiles here anyway): a lane's offset inside a (tile, 32-channel pair) never changes -- lp[view]: pixel row 0
  // of its four; rows 1-3 through the scalar offset operand, which the range check ignores -- and the work item enters
  // through the descriptor's base address.  Scalar arithmetic per item instead of ~25 vector instructions per store in
  // an epilogue that all eight waves run together (stamps: 10-20 % of a 128/256-channel layer's launch).
  const bool dense = BNBWD || P.pdma_dense != 0;
  unsigned lp[2];
#pragma unroll
  for (int q = 0; q < 2; ++q)
    lp[q] = (unsigned)((((wpx * 4) * P.dst[q].W + l15) * P.dst[q].C + (kb & 1) * 16 + (kb >> 1) * 8) * 2);
  float stat_tot = 0.f;
  float bs[C::CT][4], bq[C::CT][4];
#pragma unroll
  for (int ct = 0; ct < C::CT; ++ct)
#pragma unroll
    for (int j = 0; j < 4; ++j) { bs[ct][j] = 0.f; bq[ct][j] = 0.f; }
  for (int wk = logical; wk < total; wk += G) {
    int cot, tile;
    pdma_item(wk, n_tiles, P.co_il, cot, tile);
    const int n = tile / tiles_img, r = tile - n * tiles_img;
    const int tyi = r / P.tilesX, txi = r - tyi * P.tilesX;
    const int ty0 = tyi * C::TH, tx0 = txi * C::TW;
    const int co0 = cot * BN;
    const unsigned c_wbase = d_wbase;             // this work item's weights (DMA side moves on in the last chunk)
    const bool has_next = wk + G < total;
#pragma unroll
    for (int a = 0; a < C::CT; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[a][b][q] = 0.f;

    if constexpr (PAIR) {
      // 9 steps of two taps; chunk 0 lives in patch buffer 0, chunk 1 in buffer 1 (nchunks == 2: the launcher's condition).
      // Patch pieces: steps 0-3 bring THIS item's chunk 1 (2, 2, 2, 1 pieces per wave), steps 5-8 the NEXT item's chunk 0
      // (buffer 0 is read for the last time by step 4); the weights of step d + 2 follow the pieces of step d.
#pragma unroll
      for (int d = 0; d < 9; ++d) {
        constexpr int NPIECE[9] = {2, 2, 2, 1, 0, 2, 2, 2, 1};
        if (d == 5) {                              // from here on the DMA stream belongs to the next work item
          d_live = has_next;
          if (has_next) setup_dma(wk + G);
        }
        // W(d) was issued two steps ago; younger: the previous step's patch pieces + NDW weight DMAs [+ the output stores of
        // the previous item's epilogue].  Step 4 also needs chunk 1's LAST patch piece, issued in step 3 in front of W(5)
        if (d == 0) {
          if (after_epilogue) {
            if (P.stats) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NDW + C::NST + 1) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NDW + C::NST) : "memory");
          } else {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NDW) : "memory");
          }
        } else if (d == 4) {
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NDW) : "memory");
        } else {
          const int np = NPIECE[d == 0 ? 0 : d - 1];
          if (np == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NDW + 2) : "memory");
          else if (np == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NDW + 1) : "memory");
          else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NDW) : "memory");
        }
        __builtin_amdgcn_s_barrier();
        auto issue_dma = [&]() {
          const int first = d < 4 ? 2 * d : 2 * (d - 5);           // (steps 0-3 / 5-8: pieces 0,1 | 2,3 | 4,5 | 6)
#pragma unroll
          for (int q = 0; q < NPIECE[d]; ++q) {
            if (d < 4) dma_patch(1, first + q, 1, true);
            else dma_patch(0, first + q, 0, d_live);
          }
          if (d + 2 < 9) dma_w2(c_wbase, 2 * (d + 2), (d + 2) % 3, true);
          else dma_w2(d_wbase, 2 * (d + 2 - 9), (d + 2) % 3, d_live);
        };
        if (!late_dma) issue_dma();
        const int sA = 2 * d, sB = 2 * d + 1;
        const int cA = sA / 9, tA = sA % 9, cB = sB / 9, tB = sB % 9;
        compute2(C::A_BASE + cA * C::A_BYTES, (tA / 3) * C::RS + (tA % 3) * C::PSTR,
                 C::A_BASE + cB * C::A_BYTES, (tB / 3) * C::RS + (tB % 3) * C::PSTR, d % 3);
        if (late_dma) issue_dma();
      }
    } else
    for (int c = 0; c < nchunks; ++c) {
      const bool last = c + 1 == nchunks;
      if (last) {                                  // from here on the DMA stream belongs to the next work item
        d_live = has_next;
        if (has_next) setup_dma(wk + G);
      }
      const int pbuf = C::A_BASE + pbuf_i * C::A_BYTES;
      if constexpr (PP) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          // ---- LOAD
          clk.resume(5);
          load_frags(pbuf, (tap / 3) * C::RS + (tap % 3) * C::PSTR, tap % 3);
          __builtin_amdgcn_sched_barrier(0);
          clk.add(4, clk.now() - clk.last());
          if (tap < C::NDA) dma_patch(last ? 0 : c + 1, tap, pbuf_i ^ 1, last ? d_live : true);
          if (tap + 2 < 9) dma_w(c_wbase, c, tap + 2, (tap + 2) % 3, true);
          else if (!last) dma_w(c_wbase, c + 1, tap + 2 - 9, (tap + 2) % 3, true);
          else dma_w(d_wbase, 0, tap + 2 - 9, (tap + 2) % 3, d_live);
          // everything older than THIS phase's DMAs has landed: the next step's weight slab (issued one step ago) and,
          // by then, every patch piece of the next chunk [the previous work item's output stores sit in between]
          clk.mark(0);
          if (tap == 0 && c == 0 && after_epilogue) {                  // (tap 0 always carries a patch piece)
            if (P.stats) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(1 + C::NDW + C::NST + 1) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(1 + C::NDW + C::NST) : "memory");
          } else if (tap < C::NDA) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(1 + C::NDW) : "memory");
          } else {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NDW) : "memory");
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          clk.mark(1);
          __builtin_amdgcn_sched_barrier(0);
          __builtin_amdgcn_s_barrier();
          __builtin_amdgcn_sched_barrier(0);
          clk.mark(2);
          // ---- COMPUTE
          __builtin_amdgcn_s_setprio(1);
          mma_frags();
          __builtin_amdgcn_s_setprio(0);
          __builtin_amdgcn_sched_barrier(0);
          clk.mark(3);
          clk.tick();
          __builtin_amdgcn_s_barrier();
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        clk.resume(3);
        // W(step) was issued two steps ago; younger: the previous step's [patch DMA] + NDW weight DMAs
        // [+ the NST (+1) output stores of the previous work item's epilogue]
        if (tap == 0 && c == 0 && after_epilogue) {
          if (P.stats) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NDW + C::NST + 1) : "memory");
          else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NDW + C::NST) : "memory");
        } else if (tap == 0 || tap == 8) {
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NDW) : "memory");          // previous tap 8 / 7: no patch DMA
        } else {
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NDW + 1) : "memory");
        }
        clk.mark(0);
        __builtin_amdgcn_s_barrier();
        clk.mark(1);
        // This tap's DMA issues (a patch piece of the next chunk, the weight slab two taps ahead).  The two waves of a SIMD
        // (w, w + 4) issue at opposite ends of the tap -- waves 4-7 here, waves 0-3 behind their MFMAs -- so that one of
        // them has MFMAs to issue while the other sits in its burst (+3..8 % on these layers over all eight behind the
        // barrier, profiles/r03_pdma_stagger.txt).  The per-wave ORDER of vector-memory operations is unchanged, so every
        // counted vmcnt above still holds; a slot is refilled after the barrier that follows its last reads either way.
        auto issue_dma = [&]() {
          if (tap < C::NDA) dma_patch(last ? 0 : c + 1, tap, pbuf_i ^ 1, last ? d_live : true);
          if (tap + 2 < 9) dma_w(c_wbase, c, tap + 2, (tap + 2) % 3, true);
          else if (!last) dma_w(c_wbase, c + 1, tap + 2 - 9, (tap + 2) % 3, true);
          else dma_w(d_wbase, 0, tap + 2 - 9, (tap + 2) % 3, d_live);
        };
        if (!late_dma) issue_dma();
        clk.mark(2);
        clk.tick();
        compute(pbuf, (tap / 3) * C::RS + (tap % 3) * C::PSTR, tap % 3);
        if (late_dma) issue_dma();
      }
      }
      pbuf_i ^= 1;
    }

    const unsigned long long t_epi = clk.now();
    if (!PP) clk.add(3, t_epi - clk.last());
    clk.pause();
    // ---- epilogue: D of 16x16x32: col = lane&15 (pixel), rows (lane>>4)*4 + reg (4 consecutive channels).
    // Buffer stores (out-of-range offset = dropped) so every lane issues exactly NST of them.
    __amdgpu_buffer_rsrc_t drs[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const DViewW D = P.dst[q];
      const unsigned dimg = (unsigned)D.H * D.W * D.C * 2u;
      drs[q] = __builtin_amdgcn_make_buffer_rsrc((void*)(D.p ? D.p + (size_t)n * dimg : P.dst[0].p), (short)0,
                                                 D.p ? (int)dimg : 0, 0x00020000);
    }
    if constexpr (!DEFER) {
#pragma unroll
      for (int ct = 0; ct < C::CT; ++ct)
#pragma unroll
        for (int j = 0; j < 4; ++j) { bs[ct][j] = 0.f; bq[ct][j] = 0.f; }
    }
    if constexpr (BNBWD) {
      // dgrad + ReLU mask + BatchNorm-backward sums of the producing layer.  dst[0] is dense and frame-sized, so the
      // store offset of a (pixel, tile pair) is also the offset of its 8 y values; y comes in with the same 16-byte
      // loads as the gradient fan-in's old values and is un-swapped to the accumulator layout.  ALL loads of the work
      // item are issued before the first use: one exposed memory round trip per item.
      const DViewW D = P.dst[0];
      const unsigned dimg = (unsigned)D.H * D.W * D.C * 2u;
      const __amdgpu_buffer_rsrc_t yrs =
          __builtin_amdgcn_make_buffer_rsrc((void*)(P.bn_y + (size_t)n * dimg), (short)0, (int)dimg, 0x00020000);
      u32x4 yraw[4][C::CT / 2];
      f32x4 csc[C::CT / 2][2], csh[C::CT / 2][2], cmu[C::CT / 2][2];
      (void)yrs;
      const unsigned rowb = (unsigned)(D.W * D.C * 2);
      __amdgpu_buffer_rsrc_t yrs_c[C::CT / 2], drs_c[C::CT / 2];
#pragma unroll
      for (int cp = 0; cp < C::CT / 2; ++cp) {
        const int cw = co0 + wco * (BN / 2) + cp * 32;
        const unsigned off = (unsigned)(((ty0 * D.W + tx0) * D.C + cw) * 2);
        yrs_c[cp] = __builtin_amdgcn_make_buffer_rsrc((void*)(P.bn_y + (size_t)n * dimg + off), (short)0, (int)(dimg - off), 0x00020000);
        drs_c[cp] = __builtin_amdgcn_make_buffer_rsrc((void*)(D.p + (size_t)n * dimg + off), (short)0, (int)(dimg - off), 0x00020000);
      }
#pragma unroll
      for (int pt = 0; pt < 4; ++pt)
#pragma unroll
        for (int cp = 0; cp < C::CT / 2; ++cp) yraw[pt][cp] = __builtin_amdgcn_raw_buffer_load_b128(yrs_c[cp], lp[0], pt * rowb, 0);
#pragma unroll
      for (int cp = 0; cp < C::CT / 2; ++cp) {
        const int cw = co0 + wco * (BN / 2) + cp * 32 + kb * 4;   // native layout: tile 2cp rows kb*4.., +16: tile 2cp+1
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          csc[cp][t] = *reinterpret_cast<const f32x4*>(P.bn_scale + cw + 16 * t);
          csh[cp][t] = *reinterpret_cast<const f32x4*>(P.bn_shift + cw + 16 * t);
          cmu[cp][t] = *reinterpret_cast<const f32x4*>(P.bn_mean + cw + 16 * t);
        }
      }
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) {
#pragma unroll
        for (int cp = 0; cp < C::CT / 2; ++cp) {
          const u32x4 o = yraw[pt][cp];
          const auto o0 = __builtin_amdgcn_permlane16_swap(o[0], o[2], false, false);
          const auto o1 = __builtin_amdgcn_permlane16_swap(o[1], o[3], false, false);
          const bf16x4 ya = __builtin_bit_cast(bf16x4, u32x2{o0[0], o1[0]});
          const bf16x4 yb = __builtin_bit_cast(bf16x4, u32x2{o0[1], o1[1]});
          bf16x4 ra, rb;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float fa = (float)ya[j], fb = (float)yb[j];
            const bool ona = fmaf(fa, csc[cp][0][j], csh[cp][0][j]) > 0.f;
            const bool onb = fmaf(fb, csc[cp][1][j], csh[cp][1][j]) > 0.f;
            ra[j] = (bf16_t)(ona ? acc[2 * cp][pt][j] : 0.f);
            rb[j] = (bf16_t)(onb ? acc[2 * cp + 1][pt][j] : 0.f);
            const float qa = (float)ra[j], qb = (float)rb[j];       // dz as stored (an OOB pixel loads y = 0 and is
            bs[2 * cp][j] += qa;                                    //  dropped by its store: frames are 16-aligned here,
            bq[2 * cp][j] = fmaf(qa, fa - cmu[cp][0][j], bq[2 * cp][j]);   // so that never happens)
            bs[2 * cp + 1][j] += qb;
            bq[2 * cp + 1][j] = fmaf(qb, fb - cmu[cp][1][j], bq[2 * cp + 1][j]);
          }
          const u32x2 ua = __builtin_bit_cast(u32x2, ra), ub = __builtin_bit_cast(u32x2, rb);
          const auto s0 = __builtin_amdgcn_permlane16_swap(ua[0], ub[0], false, false);
          const auto s1 = __builtin_amdgcn_permlane16_swap(ua[1], ub[1], false, false);
          __builtin_amdgcn_raw_buffer_store_b128(u32x4{s0[0], s1[0], s0[1], s1[1]}, drs_c[cp], lp[0], pt * rowb, 0);
        }
      }
    } else {
    // v_permlane16_swap trades the (kb odd) rows of tile ct for the (kb even) rows of tile ct+1: afterwards lane kb
    // holds 8 CONSECUTIVE channels -- tile ct + (kb & 1), channels 8*(kb >> 1) .. +7 -- and writes 16 bytes (half
    // the store instructions, 64 contiguous bytes per pixel and tile pair).  Old values for the gradient fan-in
    // come in with the same 16-byte loads and are un-swapped (the exchange is an involution) before the fp32 add.
    // (pt, cp): the wave's pixel row and 32-channel tile pair; rs / vo / so: descriptor, lane offset, scalar offset of its store
    auto finish = [&](int pt, int cp, int cw, bool second, int accq, __amdgpu_buffer_rsrc_t rs, unsigned vo, unsigned so, bool ok) {
      float va[4], vb[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { va[j] = acc[2 * cp][pt][j]; vb[j] = acc[2 * cp + 1][pt][j]; }
      if (P.bias) {                                // inference: BatchNorm shift (+ ReLU) of the folded layer
        const float* bp = P.bias + cw + kb * 4;   // native accumulator layout: tile 2cp (+16: tile 2cp+1), rows kb*4..+3
#pragma unroll
        for (int j = 0; j < 4; ++j) { va[j] += bp[j]; vb[j] += bp[16 + j]; }
      }
      if (P.relu) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { va[j] = fmaxf(va[j], 0.f); vb[j] = fmaxf(vb[j], 0.f); }
      }
      if (accq) {
        const u32x4 o = __builtin_amdgcn_raw_buffer_load_b128(rs, vo, so, 0);
        const auto o0 = __builtin_amdgcn_permlane16_swap(o[0], o[2], false, false);
        const auto o1 = __builtin_amdgcn_permlane16_swap(o[1], o[3], false, false);
        const bf16x4 oa = __builtin_bit_cast(bf16x4, u32x2{o0[0], o1[0]});
        const bf16x4 ob = __builtin_bit_cast(bf16x4, u32x2{o0[1], o1[1]});
#pragma unroll
        for (int j = 0; j < 4; ++j) { va[j] += (float)oa[j]; vb[j] += (float)ob[j]; }
      }
      bf16x4 ra, rb;
#pragma unroll
      for (int j = 0; j < 4; ++j) { ra[j] = (bf16_t)va[j]; rb[j] = (bf16_t)vb[j]; }
      const u32x2 ua = __builtin_bit_cast(u32x2, ra), ub = __builtin_bit_cast(u32x2, rb);
      const auto s0 = __builtin_amdgcn_permlane16_swap(ua[0], ub[0], false, false);
      const auto s1 = __builtin_amdgcn_permlane16_swap(ua[1], ub[1], false, false);
      __builtin_amdgcn_raw_buffer_store_b128(u32x4{s0[0], s1[0], s0[1], s1[1]}, rs, vo, so, 0);
      if (ok && P.stats) {                         // (a launch without statistics skips the 24 vector instructions per store)
#pragma unroll
        for (int j = 0; j < 4; ++j) {              // statistics of the values as STORED (bf16-rounded)
          const float qa = (float)ra[j], qb = (float)rb[j];
          bs[2 * cp][j] += qa;
          bq[2 * cp][j] = fmaf(qa, qa, bq[2 * cp][j]);
          bs[2 * cp + 1][j] += qb;
          bq[2 * cp + 1][j] = fmaf(qb, qb, bq[2 * cp + 1][j]);
        }
      }
    };
    if (dense) {
#pragma unroll
      for (int cp = 0; cp < C::CT / 2; ++cp) {
        const int cw = co0 + wco * (BN / 2) + cp * 32;               // first channel of the tile pair
        const bool second = cw >= P.dst_split;                       // uniform per (wave, pair): dst_split % 64 == 0
        const int accq = second ? (P.accumulate & 2) : (P.accumulate & 1);
        const DViewW D = second ? P.dst[1] : P.dst[0];
        const unsigned dimg = (unsigned)D.H * D.W * D.C * 2u;
        const unsigned off = (unsigned)(((ty0 * D.W + tx0) * D.C + cw - (second ? P.dst_split : 0)) * 2);
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc((void*)(D.p + (size_t)n * dimg + off), (short)0, (int)(dimg - off), 0x00020000);
        const unsigned rowb = (unsigned)(D.W * D.C * 2);
        const unsigned lpq = second ? lp[1] : lp[0];
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) finish(pt, cp, cw, second, accq, rs, lpq, pt * rowb, true);
      }
    } else {
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) {
        const int fy = ty0 + wpx * 4 + pt, fx = tx0 + l15;
        const bool pix_ok = fy < P.H && fx < P.W;
#pragma unroll
        for (int cp = 0; cp < C::CT / 2; ++cp) {
          const int cw = co0 + wco * (BN / 2) + cp * 32;               // first channel of the tile pair
          const bool second = cw >= P.dst_split;                       // uniform per (wave, pair): dst_split % 64 == 0
          const int accq = second ? (P.accumulate & 2) : (P.accumulate & 1);
          const DViewW D = second ? P.dst[1] : P.dst[0];
          const int co = cw - (second ? P.dst_split : 0) + (kb & 1) * 16 + (kb >> 1) * 8;
          const int y = fy - D.oy, x = fx - D.ox;
          const bool ok = pix_ok && y >= 0 && y < D.H && x >= 0 && x < D.W;
          const unsigned vo = ok ? (unsigned)(((y * D.W + x) * D.C + co) * 2) : OOB;
          if (second) finish(pt, cp, cw, true, accq, drs[1], vo, 0u, ok);
          else finish(pt, cp, cw, false, accq, drs[0], vo, 0u, ok);
        }
      }
    }
    }
    if (P.stats) {
      // exactly one (possibly dropped) statistics store per work item: static vmcnt counts
      int ncot = cot, ntile_ = 0;
      if (has_next) pdma_item(wk + G, n_tiles, P.co_il, ncot, ntile_);
      (void)ntile_;
      const bool flush = !P.zdiv || !has_next || ncot != cot;
      // block mode: the co_il blocks that share a super-group's pixel tiles own different channel tiles -> ONE partial row
      const int part = P.zdiv ? logical / P.co_il : (n * P.tilesY + tyi) * P.tilesX + txi;
      float tsum = 0.f;
      unsigned so = OOB;
      if (!DEFER || flush) {
        {
          float rv[2 * C::CT * 4];
#pragma unroll
          for (int ct = 0; ct < C::CT; ++ct)
#pragma unroll
            for (int j = 0; j < 4; ++j) { rv[ct * 4 + j] = bs[ct][j]; rv[C::CT * 4 + ct * 4 + j] = bq[ct][j]; }
          row16_sum_n(rv);
#pragma unroll
          for (int ct = 0; ct < C::CT; ++ct)
#pragma unroll
            for (int j = 0; j < 4; ++j) { bs[ct][j] = rv[ct * 4 + j]; bq[ct][j] = rv[C::CT * 4 + ct * 4 + j]; }
        }
        float* red = reinterpret_cast<float*>(smem + C::RED_BASE);     // [4 pixel-waves][2][BN]
        if (l15 == 0) {
#pragma unroll
          for (int ct = 0; ct < C::CT; ++ct)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int cl = wco * (BN / 2) + ct * 16 + kb * 4 + j;
              red[(wpx * 2 + 0) * BN + cl] = bs[ct][j];
              red[(wpx * 2 + 1) * BN + cl] = bq[ct][j];
            }
        }
#pragma unroll
        for (int ct = 0; ct < C::CT; ++ct)
#pragma unroll
          for (int j = 0; j < 4; ++j) { bs[ct][j] = 0.f; bq[ct][j] = 0.f; }
        // LDS-only exchange: raw barrier (a __syncthreads() would also wait for the output stores)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        // PP: that barrier is this half's own exchange (the other half is a barrier apart); a half owns BN/2 channels
        // outright, so its BN threads (statistic, channel) total the four pixel-waves of THEIR half
        const int st_t = PP ? (tid & 255) : tid;
        if (st_t < (PP ? BN : 2 * BN)) {
          const int q = PP ? st_t / (BN / 2) : st_t / BN;
          const int cl = PP ? grp * (BN / 2) + st_t % (BN / 2) : st_t - q * BN;
#pragma unroll
          for (int wp = 0; wp < 4; ++wp) tsum += red[(wp * 2 + q) * BN + cl];   // fixed order: deterministic
          if (!DEFER && P.zdiv) {
            stat_tot += tsum;
            tsum = stat_tot;
            if (flush) stat_tot = 0.f;
          }
          if (flush) so = (unsigned)((((size_t)part * 2 + q) * P.Cout + co0 + cl) * 4);
        }
      }
      const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(
          (void*)P.stats, (short)0, (int)std::min<long long>((long long)n_tiles * 2 * P.Cout * 4, 0x7FFFFFFFLL), 0x00020000);
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, tsum), srs, so, 0, 0);
    }
    after_epilogue = true;
    if (!PP) clk.add(4, clk.now() - t_epi);
  }
  clk.store(STAMP_SINK(P.stamps), 8, clk.ticks());
  if constexpr (PP) { if (!grp) __builtin_amdgcn_s_barrier(); }        // pairs with the stagger barrier of waves 4-7
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // drain the dummy DMAs before the wave ends
}

__global__ __launch_bounds__(512, 1) void conv3_pdma128_kernel(const IgemmParams P) { conv3_pdma_body<128>(P); }
__global__ __launch_bounds__(512, 1) void conv3_pdma64_kernel(const IgemmParams P) { conv3_pdma_body<64>(P); }
__global__ __launch_bounds__(512, 1) void conv3_pdma128_bnbwd_kernel(const IgemmParams P) { conv3_pdma_body<128, true>(P); }
__global__ __launch_bounds__(512, 1) void conv3_pdma64_bnbwd_kernel(const IgemmParams P) { conv3_pdma_body<64, true>(P); }
__global__ __launch_bounds__(512, 1) void conv3_pp128_kernel(const IgemmParams P) { conv3_pdma_body<128, false, true>(P); }
__global__ __launch_bounds__(512, 1) void conv3_pp64_kernel(const IgemmParams P) { conv3_pdma_body<64, false, true>(P); }
__global__ __launch_bounds__(512, 1) void conv3_pp128_bnbwd_kernel(const IgemmParams P) { conv3_pdma_body<128, true, true>(P); }
__global__ __launch_bounds__(512, 1) void conv3_pp64_bnbwd_kernel(const IgemmParams P) { conv3_pdma_body<64, true, true>(P); }
__global__ __launch_bounds__(512, 1) void conv3_pdma64x2_kernel(const IgemmParams P) { conv3_pdma_body<64, false, false, true>(P); }
__global__ __launch_bounds__(512, 1) void conv3_pdma64x2_bnbwd_kernel(const IgemmParams P) { conv3_pdma_body<64, true, false, true>(P); }

template <int BN>
int32_t launch_pdma(const IgemmParams& Pin, int kclass, hipStream_t s, int* stat_parts) {
  using C = CfgP<BN>;
  IgemmParams P = Pin;
  P.nCo = P.Cout / BN;
  P.tilesX = cdiv(P.W, C::TW);
  P.tilesY = cdiv(P.H, C::TH);
  const bool bnbwd = P.bn_y != nullptr;
  P.pdma_stagger = 1;
  P.pdma_dense = 1;
  P.pdma_dense_src = 1;
  for (int k = 0; k < 2; ++k)
    if (P.src[k].p && P.src[k].C > 0 && (!covers_frame(P.src[k], P) || P.src[k].C != P.src[0].C)) P.pdma_dense_src = 0;
  for (int q = 0; q < 2; ++q)
    if (P.dst[q].p && !covers_frame(P.dst[q], P)) P.pdma_dense = 0;
  // the ping-pong schedule wins where a work item is long (>= 8 chunks: +2 % at 512, +6 % at 1024 input channels) and
  // loses where the epilogue -- run once per half, each exposed -- is a large part of an item (-10 % at 128 channels)
  const bool pp = BN == 128 && P.Ctot >= 512;
  // two taps per step for 64-channel tiles over exactly two chunks
  const bool pair = BN == 64 && P.Ctot == 128;
  auto kern = pair ? (bnbwd ? conv3_pdma64x2_bnbwd_kernel : conv3_pdma64x2_kernel)
              : pp ? (bnbwd ? (BN == 128 ? conv3_pp128_bnbwd_kernel : conv3_pp64_bnbwd_kernel)
                            : (BN == 128 ? conv3_pp128_kernel : conv3_pp64_kernel))
                   : (bnbwd ? (BN == 128 ? conv3_pdma128_bnbwd_kernel : conv3_pdma64_bnbwd_kernel)
                            : (BN == 128 ? conv3_pdma128_kernel : conv3_pdma64_kernel));
  const int lds_bytes = pair ? CfgP<64, true>::LDS : C::LDS;
  unet_set_max_lds(reinterpret_cast<const void*>(kern), lds_bytes);
  const long long work = (long long)P.N * P.tilesY * P.tilesX * P.nCo;
  UNET_REQUIRE(work > 0 && work < (1LL << 30), UNET_ERR_UNSUPPORTED, "conv3_pdma: %lld work items", work);
  const long long stat_bytes = (long long)P.N * P.tilesY * P.tilesX * 2 * P.Cout * 4;
  if (stat_bytes >= 0x7FFFFFFFLL) {
    UNET_REQUIRE(!bnbwd, UNET_ERR_UNSUPPORTED, "conv3_pdma: partial-sum buffer of %lld bytes", stat_bytes);
    P.stats = nullptr;
  }
  const int blocks = (int)std::min<long long>(unet_cu_budget(), cdiv64(work, 8) * 8);   // one per (non-reserved) CU, a multiple of 8 (XCDs)
  const double flops = 2.0 * P.N * P.H * P.W * (double)P.Cout * P.Ctot * 9;
  const long long n_tiles = (long long)P.N * P.tilesY * P.tilesX;
  // channel tiles interleaved per pixel tile: up to 4
  P.co_il = 1;
  while (P.co_il * 2 <= 4 && P.nCo % (P.co_il * 2) == 0 && blocks % (P.co_il * 2 * 8) == 0) P.co_il *= 2;
  // block-mode statistics: a block stays on one channel tile for whole super-groups and the co_il blocks of a row cover them all
  P.zdiv = (P.stats && (n_tiles * P.co_il) % blocks == 0) ? 1 : 0;
  if (P.stats && stat_parts) *stat_parts = P.zdiv ? blocks / P.co_il : (int)n_tiles;
#ifdef PDMA_STAMPS
  P.stamps = g_stamp_sink;
#endif
  // (one bracket name per body: the lock-step and ping-pong instantiations of conv3_pdma_body<BN> are one kernel family)
  // algorithmic bytes: input + packed weights + output, each once (+ y of the fused BatchNorm-backward form, + the old
  // values of an accumulating epilogue), bf16
  const double px = (double)P.N * P.H * P.W;
  const double alg_bytes = 2.0 * (px * (P.Ctot + P.Cout * (1.0 + (bnbwd ? 1 : 0) + (P.accumulate ? 1 : 0))) + 9.0 * P.Ctot * P.Cout);
  ProfScope prof(kclass, flops, s, bnbwd ? (BN == 128 ? "conv3_pdma128_bnbwd_kernel" : "conv3_pdma64_bnbwd_kernel")
                                          : (BN == 128 ? "conv3_pdma128_kernel" : "conv3_pdma64_kernel"), alg_bytes);
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(512), lds_bytes, s, P);
  return unet_check_launch("conv3_pdma_kernel");
}

}  // namespace

int32_t unet_internal_conv3_pdma(const IgemmParams& P, int kclass, hipStream_t s, int* stat_parts) {
  return P.Cout % 128 == 0 ? launch_pdma<128>(P, kclass, s, stat_parts) : launch_pdma<64>(P, kclass, s, stat_parts);
}
