// Full-resolution prediction (predict_tiled; no reference counterpart: the reference squeezes every image into the
// trainer's frame): a large frame is cut into overlapping tiles the model runs at its trained size, and the tile logits
// are recombined into one label map and one confidence map without seams.
//   tile_gather   tiles[t][c][ky][kx] = frame[c][oy[i] + ky][ox[j] + kx], t = i * nx + j: a copy, one launch per image
//   tile_blend    per frame pixel, over the tiles that cover it in ascending i, then ascending j:
//                   q(k) = min(k + 1, L - k, B) along each axis (tile length L, ramp B), the tile's weight q_y * q_x,
//                   wsum += q_y * q_x (int32),  acc_c = acc_c + (float)(q_y * q_x) * z_c  (product and sum rounded apart:
//                   this file is built with -ffp-contract=off),  blended_c = acc_c / (float)wsum;
//                 a pixel under exactly one tile takes that tile's logits unchanged.  labels / conf follow from the
//                 blended logits by segpixel.h's argmax_conf (first maximum; 1 / sum_j expf(z_j - max z), j in class
//                 order): the one rule seg_confidence applies to raw logits, so the two agree bit for bit.
// The gather form: a lane owns output pixels and walks the tiles over them; no atomics, no LDS, the outputs are a
// function of the inputs alone.  The origin tables (at most 64 per axis) travel in the kernel arguments.  A block works
// on a segment of ONE row, so everything along y -- the covering tiles, q_y -- is wave-uniform, and the tables are only
// ever indexed by uniform loop counters (scalar loads from the argument segment); along x every lane tests the nx tiles.
// A lane owns 4 consecutive x (16-byte loads and stores) when w, tw and every ox[j] are multiples of 4 and the pointers
// are aligned: the four pixels then lie under the same tiles.  Else one pixel.  HBM-bound: every tile logit is read once.
#include "segpixel.h"

namespace {

using namespace segpx;                                 // MAXC, aligned, argmax_conf (segpixel.h)
constexpr int MAX_TILES_AXIS = 64;
constexpr int MAX_RAMP = 256;
constexpr int TL_THREADS = 256;
constexpr int TL_MAX_BLOCKS = 4096;

struct TileGrid {
  int oy[MAX_TILES_AXIS], ox[MAX_TILES_AXIS];
  int ny, nx, th, tw;                                  // tiles per axis, tile size
  int c, h, w;                                         // frame
  int segs;                                            // blocks' segments per row: cdiv(units per row, blockDim.x)
  long long items;                                     // row segments of the launch
};

struct BlendParams {
  const float* tiles; unsigned char* labels; float* conf; float* blended;
  int ramp_y, ramp_x;
};

__device__ __forceinline__ int ramp_weight(int k, int L, int B) { return min(min(k + 1, L - k), B); }

// item = row of the tile buffer ((t * c + ch) * th + ky) x segment: the source row is uniform
template <int V>
__global__ __launch_bounds__(TL_THREADS) void tile_gather(const TileGrid G, const float* __restrict__ frame,
                                                          float* __restrict__ tiles) {
  for (long long item = blockIdx.x; item < G.items; item += gridDim.x) {
    const long long row = item / G.segs;
    const int kx = ((int)(item % G.segs) * (int)blockDim.x + (int)threadIdx.x) * V;
    if (kx >= G.tw) continue;
    const int ky = (int)(row % G.th);
    const long long plane = row / G.th;
    const int ch = (int)(plane % G.c), t = (int)(plane / G.c);
    const int y = G.oy[t / G.nx] + ky, x = G.ox[t % G.nx] + kx;
    const float* src = frame + ((long long)ch * G.h + y) * G.w + x;
    float* dst = tiles + row * G.tw + kx;
    if constexpr (V == 4) *reinterpret_cast<f32x4*>(dst) = *reinterpret_cast<const f32x4*>(src);
    else *dst = *src;
  }
}

// item = frame row y x segment; CM = 4 or 8 class slots in registers (up to 4 classes run at twice the occupancy)
template <int V, int CM>
__global__ __launch_bounds__(TL_THREADS) void tile_blend(const TileGrid G, const BlendParams P) {
  const long long tile_plane = (long long)G.th * G.tw, frame_plane = (long long)G.h * G.w;
  for (long long item = blockIdx.x; item < G.items; item += gridDim.x) {
    const int y = (int)(item / G.segs);
    const int x = ((int)(item % G.segs) * (int)blockDim.x + (int)threadIdx.x) * V;
    if (x >= G.w) continue;
    float acc[CM][V], one[CM][V];                  // the weighted sums; the logits of the first covering tile
    int wsum[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      wsum[v] = 0;
#pragma unroll
      for (int c = 0; c < CM; ++c) acc[c][v] = one[c][v] = 0.f;
    }
    int covers = 0;
    for (int i = 0; i < G.ny; ++i) {
      const int ky = y - G.oy[i];
      if (ky < 0 || ky >= G.th) continue;              // uniform
      const int qy = ramp_weight(ky, G.th, P.ramp_y);
      for (int j = 0; j < G.nx; ++j) {
        const int kx = x - G.ox[j];
        if (kx < 0 || kx >= G.tw) continue;            // V == 4: kx and tw are multiples of 4, the four pixels agree
        const float* zt = P.tiles + ((long long)(i * G.nx + j) * G.c) * tile_plane + (long long)ky * G.tw + kx;
        float qf[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const int q = qy * ramp_weight(kx + v, G.tw, P.ramp_x);
          wsum[v] += q;
          qf[v] = (float)q;
        }
#pragma unroll
        for (int c = 0; c < CM; ++c) {
          if (c < G.c) {
            float z[V];
            if constexpr (V == 4) {
              const f32x4 t4 = *reinterpret_cast<const f32x4*>(zt + c * tile_plane);
              z[0] = t4[0]; z[1] = t4[1]; z[2] = t4[2]; z[3] = t4[3];
            } else {
              z[0] = zt[c * tile_plane];
            }
#pragma unroll
            for (int v = 0; v < V; ++v) {
              if (covers == 0) one[c][v] = z[v];
              const float p = qf[v] * z[v];
              acc[c][v] = acc[c][v] + p;
            }
          }
        }
        ++covers;
      }
    }
    // a valid cover leaves no pixel bare: covers >= 1, wsum >= 1
    int arg[V];
    float cf[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const float ws = (float)wsum[v];
      float z[CM];
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        z[c] = c < G.c ? (covers == 1 ? one[c][v] : acc[c][v] / ws) : 0.f;
        acc[c][v] = z[c];
      }
      arg[v] = argmax_conf(z, G.c, cf[v]);
    }
    const long long o = (long long)y * G.w + x;
    if constexpr (V == 4) {
      if (P.labels)
        *reinterpret_cast<unsigned int*>(P.labels + o) =
            (unsigned)arg[0] | ((unsigned)arg[1] << 8) | ((unsigned)arg[2] << 16) | ((unsigned)arg[3] << 24);
      if (P.conf) {
        const f32x4 t4 = {cf[0], cf[1], cf[2], cf[3]};
        *reinterpret_cast<f32x4*>(P.conf + o) = t4;
      }
      if (P.blended) {
#pragma unroll
        for (int c = 0; c < CM; ++c)
          if (c < G.c) {
            const f32x4 t4 = {acc[c][0], acc[c][1], acc[c][2], acc[c][3]};
            *reinterpret_cast<f32x4*>(P.blended + c * frame_plane + o) = t4;
          }
      }
    } else {
      if (P.labels) P.labels[o] = (unsigned char)arg[0];
      if (P.conf) P.conf[o] = cf[0];
      if (P.blended) {
#pragma unroll
        for (int c = 0; c < CM; ++c)
          if (c < G.c) P.blended[c * frame_plane + o] = acc[c][0];
      }
    }
  }
}

// the origins of one axis are a cover of [0, F) by tiles of length L: first 0, last F - L, strictly increasing, no gap
bool valid_cover(const int32_t* o, int n, int F, int L) {
  if (o[0] != 0 || o[n - 1] != F - L) return false;
  for (int k = 1; k < n; ++k)
    if (o[k] <= o[k - 1] || o[k] - o[k - 1] > L) return false;
  return true;
}

// The shape limits both entry points share (UNET_ERR_UNSUPPORTED), then the tables (UNET_ERR_BAD_ARG); fills G but for
// segs / items.  With a valid cover every oy[i] + ky < h and ox[j] + kx < w, and t < ny nx: no table can send a kernel
// outside the frame or the tile buffer.
int32_t tile_grid(const char* who, int c, int h, int w, int th, int tw, const int32_t* oy, int ny, const int32_t* ox, int nx,
                  bool pointers, TileGrid& G, bool& vec) {
  UNET_REQUIRE(ny >= 1 && ny <= MAX_TILES_AXIS && nx >= 1 && nx <= MAX_TILES_AXIS, UNET_ERR_UNSUPPORTED,
               "%s: %d x %d tiles (1..%d per axis)", who, ny, nx, MAX_TILES_AXIS);
  UNET_REQUIRE(h >= 1 && w >= 1 && th >= 1 && th <= h && tw >= 1 && tw <= w, UNET_ERR_UNSUPPORTED,
               "%s: tiles of %d x %d in a frame of %d x %d (1 <= tile <= frame)", who, th, tw, h, w);
  UNET_REQUIRE((long long)h * w <= 2147483647LL, UNET_ERR_UNSUPPORTED,
               "%s: a frame of %d x %d pixels (at most 2^31 - 1)", who, h, w);
  UNET_REQUIRE(pointers && oy && ox, UNET_ERR_BAD_ARG, "%s: null pointer", who);
  UNET_REQUIRE(valid_cover(oy, ny, h, th) && valid_cover(ox, nx, w, tw), UNET_ERR_BAD_ARG,
               "%s: the origins are not a cover (first 0, last frame - tile, increasing, gaps <= tile)", who);
  vec = w % 4 == 0 && tw % 4 == 0;
  for (int i = 0; i < ny; ++i) G.oy[i] = oy[i];
  for (int j = 0; j < nx; ++j) { G.ox[j] = ox[j]; vec = vec && ox[j] % 4 == 0; }
  G.ny = ny; G.nx = nx; G.th = th; G.tw = tw; G.c = c; G.h = h; G.w = w;
  return UNET_OK;
}

// block = the row's units rounded up to whole waves, at most TL_THREADS; grid-stride over the row segments
void tile_launch_shape(TileGrid& G, int units_per_row, long long rows, unsigned& blocks, unsigned& threads) {
  threads = (unsigned)(cdiv(units_per_row, WAVE) * WAVE);
  if (threads > TL_THREADS) threads = TL_THREADS;
  G.segs = cdiv(units_per_row, (int)threads);
  G.items = rows * G.segs;
  blocks = (unsigned)(G.items < TL_MAX_BLOCKS ? G.items : TL_MAX_BLOCKS);
}

}  // namespace

extern "C" int32_t unet_tile_gather(const float* frame, int32_t c, int32_t h, int32_t w, int32_t th, int32_t tw,
                                    const int32_t* oy, int32_t ny, const int32_t* ox, int32_t nx, float* tiles,
                                    void* stream) {
  const char* who = "unet_tile_gather";
  UNET_REQUIRE(c >= 1, UNET_ERR_UNSUPPORTED, "%s: c=%d (at least 1 channel)", who, c);
  TileGrid G{};
  bool vec = false;
  const int32_t rc = tile_grid(who, c, h, w, th, tw, oy, ny, ox, nx, frame && tiles, G, vec);
  if (rc) return rc;
  vec = vec && aligned(frame, 16) && aligned(tiles, 16);
  hipStream_t s = (hipStream_t)stream;
  unsigned blocks, threads;
  tile_launch_shape(G, cdiv(tw, vec ? 4 : 1), (long long)ny * nx * c * th, blocks, threads);
  ProfScope prof(UNET_K_OTHER, 0.0, s, "tile_gather", 8.0 * ny * nx * c * th * tw);
  if (vec) hipLaunchKernelGGL(tile_gather<4>, dim3(blocks), dim3(threads), 0, s, G, frame, tiles);
  else hipLaunchKernelGGL(tile_gather<1>, dim3(blocks), dim3(threads), 0, s, G, frame, tiles);
  return unet_check_launch("tile_gather");
}

extern "C" int32_t unet_tile_blend(const float* tiles, int32_t c, int32_t th, int32_t tw, const int32_t* oy, int32_t ny,
                                   const int32_t* ox, int32_t nx, int32_t h, int32_t w, int32_t ramp_y, int32_t ramp_x,
                                   uint8_t* labels, float* conf, float* blended, void* stream) {
  const char* who = "unet_tile_blend";
  UNET_REQUIRE(c >= 2 && c <= MAXC, UNET_ERR_UNSUPPORTED, "%s: c=%d (2..8 classes)", who, c);
  UNET_REQUIRE(ramp_y >= 1 && ramp_y <= MAX_RAMP && ramp_x >= 1 && ramp_x <= MAX_RAMP, UNET_ERR_UNSUPPORTED,
               "%s: ramps %d, %d (1..%d)", who, ramp_y, ramp_x, MAX_RAMP);
  TileGrid G{};
  bool vec = false;
  const int32_t rc = tile_grid(who, c, h, w, th, tw, oy, ny, ox, nx, tiles && (labels || conf), G, vec);
  if (rc) return rc;
  vec = vec && aligned(tiles, 16) && (!labels || aligned(labels, 4)) && (!conf || aligned(conf, 16)) &&
        (!blended || aligned(blended, 16));
  hipStream_t s = (hipStream_t)stream;
  unsigned blocks, threads;
  tile_launch_shape(G, cdiv(w, vec ? 4 : 1), h, blocks, threads);
  const BlendParams P{tiles, labels, conf, blended, ramp_y, ramp_x};
  const double bytes = 4.0 * ny * nx * c * th * tw +
                       (double)h * w * ((labels ? 1.0 : 0.0) + (conf ? 4.0 : 0.0) + (blended ? 4.0 * c : 0.0));
  ProfScope prof(UNET_K_OTHER, 0.0, s, "tile_blend", bytes);
  const auto kernel = vec ? (c <= 4 ? tile_blend<4, 4> : tile_blend<4, MAXC>)
                          : (c <= 4 ? tile_blend<1, 4> : tile_blend<1, MAXC>);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, s, G, P);
  return unet_check_launch("tile_blend");
}
