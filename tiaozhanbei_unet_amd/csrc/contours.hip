// Outlines of labelled class regions: the inverse of polygon.hip.  Every region of unet_label_class_regions that is kept
// (size >= min_pixels) is traced along the cracks between its pixels and the rest, and every closed loop of cracks
// becomes one row of `loops` and a run of `points`, the pixel-centre polygon that Pillow's ImageDraw.polygon fills back
// to the region with its holes closed.  tests/_contours_ref.py restates the rules one edge at a time.
//
// A directed crack edge is (pixel p, direction d), d = 0 E (+x), 1 S (+y), 2 W, 3 N: it exists when p is a member and its
// neighbour in direction r = (d + 1) % 4 is not (another region, background, outside the frame), and it is the side of p
// facing r, travelled in direction d.  Its id is 4 (y w + x) + d.  Successor: (p + d + r, r) if that pixel is a member
// (turn right, which also takes the 8-connected saddle), else (p + d, d) if that one is (straight), else (p, d - 1)
// (turn left).  The successor is an edge, the map is a bijection, the edges fall into loops.  The leader of a loop is its
// smallest id.  A loop's points are its edges' pixels with cyclic repeats merged and the points dropped whose step in
// equals their step out; the edge that ENDS a kept point carries the flag.
//
// Everything about an edge -- whether it exists, its successor, its predecessor, whether it ends a point -- follows from
// the 8 membership bits `nb` around its pixel, bit 2 d = the neighbour in direction d, bit 2 d + 1 = the diagonal
// between d and d + 1.  A step between two pixels is the bit number of the neighbour it leads to.
//
// The pixels are taken 1024 to a block over the whole batch (an image has no edge into another: membership ends at the
// frame).  The edges are compacted in ascending id: code[pixel] = its 4 edge bits and the rank of its first edge within
// the block, offs[block] = the block's first edge; the block sums are scanned by one workgroup.  On the compact arrays:
//   link_edges     successor, predecessor (scattered: a bijection), flag, own index as the running minimum
//   double_min     pointer doubling, `rounds` launches over ping-pong buffers: the minimum over 2^k successors
//   start_ranks    leader = that minimum; the loop is cut at its leader: the leader has no predecessor
//   double_sum     `rounds` launches: flags summed towards the leader, the point ordinal of every edge
//   scans          leaders -> loop index; points per loop at the leader -> first point (block sums, spine, apply)
//   write_rows, emit_points   the rows, then the points and area2 (int64 atomicAdd into the row: exact in any order)
// rounds = ceil(log2(edge_cap)) comes from the host; no kernel waits for another block and every loop is counted.  The
// positions come from prefix sums, never from an atomic: the outputs are a function of the inputs alone, bytes included.
//
// The counts need no tracing: edges and flags are counted per pixel, and the loops are 2 K - (Q1 - Q3 - 2 QD) / 4 with K
// the kept regions and Q the bit quads of their own masks (Gray 1971: regions - holes, 8-connected), one loop around
// every region and one around every hole.
#include "unionfind.h"

namespace {

using uf::up16;
constexpr int THREADS = 256;
constexpr int ITEMS = 4;
constexpr int BLOCK = THREADS * ITEMS;                 // elements per block of every pass and scan: ranks fit 12 bits
constexpr int WAVES = THREADS / WAVE;
constexpr int SPINE_THREADS = 1024;
constexpr int SPINE_WAVES = SPINE_THREADS / WAVE;
constexpr int64_t MAX_PIXELS = 1LL << 29;              // an edge id fits int32
constexpr int DEV = __HIP_MEMORY_SCOPE_AGENT;

struct Frames {
  const int* region; const int* sizes;
  int min_pixels, image_base, h, w;
  long long per, total;                                // h w, n h w
};

// the edges of this call, or 0 where they exceed what the buffers hold (nothing is traced then; the counts stand)
__device__ __forceinline__ long long live_edges(const long long* counts, long long cap) {
  const long long m = counts[0];
  return m <= cap ? m : 0;
}

__device__ __forceinline__ unsigned bit(unsigned nb, int k) { return nb >> (k & 7) & 1u; }

// membership of the 8 neighbours of the pixel `at` points to, value v
__device__ __forceinline__ unsigned around(const int* at, int v, int x, int y, int h, int w) {
  const bool up = y > 0, down = y + 1 < h, left = x > 0, right = x + 1 < w;
  unsigned nb = 0u;
  if (right && at[1] == v) nb |= 1u;
  if (right && down && at[w + 1] == v) nb |= 2u;
  if (down && at[w] == v) nb |= 4u;
  if (down && left && at[w - 1] == v) nb |= 8u;
  if (left && at[-1] == v) nb |= 16u;
  if (left && up && at[-w - 1] == v) nb |= 32u;
  if (up && at[-w] == v) nb |= 64u;
  if (up && right && at[-w + 1] == v) nb |= 128u;
  return nb;
}

// v > 0 of a kept member pixel g, else 0.  A value outside 1 .. per is no region of this frame
__device__ __forceinline__ int kept_value(const Frames& A, long long g) {
  const int v = A.region[g];
  return (v > 0 && v <= A.per && A.sizes[g] >= A.min_pixels) ? v : 0;
}

__device__ __forceinline__ unsigned edge_bits(unsigned nb) {
  unsigned m = 0u;
#pragma unroll
  for (int d = 0; d < 4; ++d) m |= (bit(nb, 2 * d + 2) ^ 1u) << d;
  return m;
}

// the step out of edge d: the neighbour its successor lies on, or -1 for a turn left (the same pixel)
__device__ __forceinline__ int step_out(unsigned nb, int d) {
  return bit(nb, 2 * d + 1) ? ((2 * d + 1) & 7) : bit(nb, 2 * d) ? 2 * d : -1;
}

// Does edge d end a kept point?  Not if its successor stays on the pixel.  Else the run of edges on this pixel began at
// most 3 turns left earlier, at the edge dc that was entered straight (step 2 dc) or by a turn right (step 2 dc - 1); the
// point stays iff that step differs from the step out.  A pixel on its own is the one point of its loop: its leader
// (d == 0) carries it.
__device__ __forceinline__ bool ends_point(unsigned nb, int d) {
  if (nb == 0u) return d == 0;
  const int out = step_out(nb, d);
  if (out < 0) return false;
  int dc = d;
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (!bit(nb, 2 * dc + 3) && !bit(nb, 2 * dc + 4)) dc = (dc + 1) & 3;      // entered by a turn left on this pixel
  const int in = bit(nb, 2 * dc + 3) ? ((2 * dc + 7) & 7) : 2 * dc;
  return in != out;
}

// Q1 - Q3 - 2 QD over the 2 x 2 windows of the region's own mask that this pixel is the first member of (order
// top-left, top-right, bottom-left, bottom-right), as shapes.hip counts them
__device__ __forceinline__ int quad_term(unsigned nb) {
  const bool e = nb & 1u, se = nb & 2u, s = nb & 4u, sw = nb & 8u, we = nb & 16u, nw = nb & 32u, no = nb & 64u, ne = nb & 128u;
  int q = 0;
  if (!nw && !no && !we) q += 1;                       // bottom-right of its window
  if (!no && !ne && !e) q += 1;                        // bottom-left
  if (!we) q += sw ? (s ? -1 : -2) : (s ? 0 : 1);      // top-right
  const int m = (int)e + (int)s + (int)se;             // top-left
  q += m == 0 ? 1 : m == 1 ? (se ? -2 : 0) : m == 2 ? -1 : 0;
  return q;
}

// s[BLOCK] holds one value per element in element order; on return it holds their exclusive prefix.  Returns the total.
// Every thread of the block calls this.
__device__ __forceinline__ int block_scan(int* s, int* wave_total) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  __syncthreads();
  int a[ITEMS], sum = 0;
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) { a[k] = s[threadIdx.x * ITEMS + k]; sum += a[k]; }
  int inc = sum;
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) { const int u = __shfl_up(inc, o); if (lane >= o) inc += u; }
  if (lane == WAVE - 1) wave_total[wave] = inc;
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int i = 0; i < WAVES; ++i) { const int t = wave_total[i]; if (i < wave) before += t; total += t; }
  int ex = before + inc - sum;
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) { s[threadIdx.x * ITEMS + k] = ex; ex += a[k]; }
  __syncthreads();
  return total;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) v += __shfl_xor(v, o);
  return v;
}

// grid: pixels of the batch / BLOCK.  code[g] = rank of the pixel's first edge within the block << 4 | its edge bits;
// sums[4][blocks] = the block's edges, point flags, kept regions (root pixels) and quad terms
__global__ __launch_bounds__(THREADS) void mark_edges(const Frames A, unsigned short* code, int* sums, int blocks) {
  __shared__ int s[BLOCK];
  __shared__ int wave_total[WAVES];
  __shared__ int part[3][WAVES];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  unsigned mask[ITEMS];
  int flags = 0, roots = 0, quads = 0;
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const long long g = (long long)blockIdx.x * BLOCK + k * THREADS + threadIdx.x;
    mask[k] = 0u;
    const int v = g < A.total ? kept_value(A, g) : 0;
    if (v) {
      const long long at = g % A.per;
      const int x = (int)(at % A.w), y = (int)(at / A.w);
      const unsigned nb = around(A.region + g, v, x, y, A.h, A.w);
      mask[k] = edge_bits(nb);
#pragma unroll
      for (int d = 0; d < 4; ++d)
        if ((mask[k] >> d & 1u) && ends_point(nb, d)) ++flags;
      if (v == at + 1) ++roots;
      quads += quad_term(nb);
    }
    s[k * THREADS + threadIdx.x] = __popc(mask[k]);
  }
  const int total = block_scan(s, wave_total);
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const long long g = (long long)blockIdx.x * BLOCK + k * THREADS + threadIdx.x;
    if (g < A.total) code[g] = (unsigned short)((unsigned)s[k * THREADS + threadIdx.x] << 4 | mask[k]);
  }
  flags = wave_sum(flags); roots = wave_sum(roots); quads = wave_sum(quads);
  if (lane == 0) { part[0][wave] = flags; part[1][wave] = roots; part[2][wave] = quads; }
  __syncthreads();
  if (threadIdx.x == 0) {
    int f = 0, r = 0, q = 0;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) { f += part[0][i]; r += part[1][i]; q += part[2][i]; }
    sums[blockIdx.x] = total;
    sums[blocks + blockIdx.x] = f;
    sums[2 * blocks + blockIdx.x] = r;
    sums[3 * blocks + blockIdx.x] = q;
  }
}

// One workgroup: offs[i] = the sum of in[0 .. i) for i < count, *total = the sum of all (where total is not NULL).  A
// thread sums `chunk` = ceil(count / SPINE_THREADS) neighbours, the threads' sums are scanned across the block.
__global__ __launch_bounds__(SPINE_THREADS) void scan_spine(const int* in, int* offs, int count, int chunk, long long* total) {
  __shared__ long long wave_total[SPINE_WAVES];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const long long first = (long long)threadIdx.x * chunk;
  long long sum = 0;
  for (int i = 0; i < chunk; ++i)
    if (first + i < count) sum += in[first + i];
  long long inc = sum;
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) { const long long u = __shfl_up(inc, o); if (lane >= o) inc += u; }
  if (lane == WAVE - 1) wave_total[wave] = inc;
  __syncthreads();
  long long before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < SPINE_WAVES; ++i) { const long long t = wave_total[i]; if (i < wave) before += t; all += t; }
  long long ex = before + inc - sum;
  for (int i = 0; i < chunk; ++i)
    if (first + i < count) { const int v = in[first + i]; offs[first + i] = (int)ex; ex += v; }
  if (total && threadIdx.x == 0) *total = all;
}

// the three counts from the spine totals {edges, flags, regions, quads} in t[4]
__global__ void finish_counts(const long long* t, long long* counts) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    counts[0] = t[0];
    counts[1] = 2 * t[2] - t[3] / 4;
    counts[2] = t[1];
  }
}

struct Edges {                                         // the compact arrays, `cap` entries each
  const unsigned short* code; const int* offs;         // of the pixels and their blocks
  const long long* counts; long long cap;
  int* gid; int* flag; int* prev;
};

__device__ __forceinline__ int slot_of(const Edges& E, long long g, int d) {
  const unsigned c = E.code[g];
  return E.offs[g / BLOCK] + (int)(c >> 4) + __popc(c & ((1u << d) - 1u));
}

// grid as mark_edges.  Edge i = slot_of(pixel, d): gid = 4 g + d over the batch, next = its successor's slot,
// prev[next] = i, lowest = i, flag
__global__ __launch_bounds__(THREADS) void link_edges(const Frames A, const Edges E, int* next, int* lowest) {
  const long long m = live_edges(E.counts, E.cap);
  if (m == 0) return;
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const long long g = (long long)blockIdx.x * BLOCK + k * THREADS + threadIdx.x;
    if (g >= A.total) continue;
    const unsigned mask = E.code[g] & 15u;
    if (!mask) continue;
    const int v = A.region[g];
    const long long at = g % A.per;
    const int x = (int)(at % A.w), y = (int)(at / A.w);
    const unsigned nb = around(A.region + g, v, x, y, A.h, A.w);
    int i = slot_of(E, g, 0);
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      if (!(mask >> d & 1u)) continue;
      const int out = step_out(nb, d);
      long long gs = g;
      int ds = (d + 3) & 3;
      if (out >= 0) {
        const int dx = (out == 0 || out == 1 || out == 7) ? 1 : (out >= 3 && out <= 5) ? -1 : 0;
        const int dy = (out >= 1 && out <= 3) ? 1 : (out >= 5) ? -1 : 0;
        gs = g + dx + (long long)dy * A.w;
        ds = (out & 1) ? ((d + 1) & 3) : d;
      }
      int j = slot_of(E, gs, ds);
      if (j < 0 || j >= m) j = i;                      // maps that are no labelling: stay inside the arrays
      if (i < m) {
        E.gid[i] = (int)(4 * g + d);
        E.flag[i] = ends_point(nb, d) ? 1 : 0;
        next[i] = j;
        lowest[i] = i;
        E.prev[j] = i;
      }
      ++i;
    }
  }
}

// grid: cap / THREADS.  One round: the minimum over twice as many successors, the pointer twice as far
__global__ __launch_bounds__(THREADS) void double_min(const long long* counts, long long cap, const int* next_in,
                                                      const int* low_in, int* next_out, int* low_out) {
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= live_edges(counts, cap)) return;
  const int j = next_in[i];
  low_out[i] = min(low_in[i], low_in[j]);
  next_out[i] = next_in[j];
}

// the loop is cut at its leader (back[i] = -1 there, else the predecessor); ranks start as the flags; lead[i] = 1 at a
// leader, for the scan that numbers the loops
__global__ __launch_bounds__(THREADS) void start_ranks(const Edges E, const int* leader, int* back, int* rank, int* lead) {
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  const long long m = live_edges(E.counts, E.cap);
  if (i >= m) return;
  const bool is_leader = leader[i] == (int)i;
  const int p = E.prev[i];                             // unwritten only where the maps are no labelling
  back[i] = (is_leader || p < 0 || p >= m) ? -1 : p;
  rank[i] = E.flag[i];
  lead[i] = is_leader ? 1 : 0;
}

// One round: the flags of twice as many predecessors, up to the leader
__global__ __launch_bounds__(THREADS) void double_sum(const long long* counts, long long cap, const int* back_in,
                                                      const int* rank_in, int* back_out, int* rank_out) {
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= live_edges(counts, cap)) return;
  const int j = back_in[i];
  rank_out[i] = rank_in[i] + (j >= 0 ? rank_in[j] : 0);
  back_out[i] = j >= 0 ? back_in[j] : -1;
}

// at a leader: the points of its loop = the rank of the last edge of the walk, its predecessor; 0 elsewhere
__global__ __launch_bounds__(THREADS) void loop_points(const Edges E, const int* leader, const int* rank, int* n_points) {
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  const long long m = live_edges(E.counts, E.cap);
  if (i >= m) return;
  const int p = E.prev[i];
  n_points[i] = (leader[i] == (int)i && p >= 0 && p < m) ? rank[p] : 0;
}

// grid: cap / BLOCK.  sums[block] = the sum of the block's live elements
__global__ __launch_bounds__(THREADS) void scan_sums(const long long* counts, long long cap, const int* in, int* sums) {
  __shared__ int part[WAVES];
  const long long m = live_edges(counts, cap);
  int v = 0;
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x * ITEMS + k;
    if (i < m) v += in[i];
  }
  v = wave_sum(v);
  if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) t += part[i];
    sums[blockIdx.x] = t;
  }
}

// out[i] = offs[block] + the sum of the block's elements before i; in == out is fine (a block reads before it writes)
__global__ __launch_bounds__(THREADS) void scan_apply(const long long* counts, long long cap, const int* in, const int* offs,
                                                      int* out) {
  __shared__ int s[BLOCK];
  __shared__ int wave_total[WAVES];
  const long long m = live_edges(counts, cap);
  const int base = offs[blockIdx.x];
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x * ITEMS + k;
    s[threadIdx.x * ITEMS + k] = i < m ? in[i] : 0;
  }
  block_scan(s, wave_total);
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x * ITEMS + k;
    if (i < m) out[i] = base + s[threadIdx.x * ITEMS + k];
  }
}

struct Rows {
  const int* leader; const int* rank; const int* loop_index; const int* first_point; const int* n_points;
  long long* loops; long long loop_cap;
  int* points; long long point_cap;
};

// a leader writes its loop's row, area2 = 0
__global__ __launch_bounds__(THREADS) void write_rows(const Frames A, const Edges E, const Rows R) {
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= live_edges(E.counts, E.cap) || R.leader[i] != (int)i) return;
  const long long k = R.loop_index[i];
  if (k >= R.loop_cap) return;
  const long long g = E.gid[i] >> 2;
  const long long image = g / A.per;
  long long* r = R.loops + k * 6;
  r[0] = A.image_base + image;
  r[1] = A.region[g] - 1;
  r[2] = E.gid[i] - 4 * image * A.per;
  r[3] = R.n_points[i];
  r[4] = R.first_point[i];
  r[5] = 0;
}

// after write_rows: every edge adds x1 y0 - x0 y1 of its corner end points to its loop's area2, and the edge that ends a
// point writes the point at first point + ordinal
__global__ __launch_bounds__(THREADS) void emit_points(const Frames A, const Edges E, const Rows R) {
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= live_edges(E.counts, E.cap)) return;
  const int lead = R.leader[i];
  const long long k = R.loop_index[lead];
  const int id = E.gid[i], d = id & 3;
  const long long at = (id >> 2) % A.per;
  const long long x = at % A.w, y = at / A.w;
  const long long x0 = x + (d >= 2), y0 = y + (d == 0 || d == 3), x1 = x + (d == 0 || d == 3), y1 = y + (d <= 1);
  if (k < R.loop_cap) __hip_atomic_fetch_add(&R.loops[k * 6 + 5], x1 * y0 - x0 * y1, __ATOMIC_RELAXED, DEV);
  if (E.flag[i]) {
    const long long p = (long long)R.first_point[lead] + R.rank[i] - 1;
    if (p < R.point_cap) { R.points[2 * p] = (int)x; R.points[2 * p + 1] = (int)y; }
  }
}

inline bool supported(int64_t n, int64_t h, int64_t w) {
  return uf::frames_supported(n, h, w) && n * h * w <= MAX_PIXELS;
}

struct Layout {                                        // byte offsets into the workspace
  size_t code, sums, offs, totals, end_count;          // the counting stage: code[pixels], sums / offs [4][blocks], totals[4]
  size_t arrays, edge_sums, edge_offs, end;            // the tracing stage: 11 int32 [cap], the scans' block sums
  int64_t blocks, edge_blocks;
};

inline Layout layout(int64_t n, int64_t h, int64_t w, int64_t cap) {
  Layout L;
  const int64_t pixels = n * h * w;
  L.blocks = cdiv64(pixels, BLOCK);
  L.edge_blocks = cdiv64(cap, BLOCK);
  size_t at = 0;
  L.code = at; at += up16((size_t)pixels * 2);
  L.sums = at; at += up16((size_t)L.blocks * 16);
  L.offs = at; at += up16((size_t)L.blocks * 16);
  L.totals = at; at += 32;
  L.end_count = at;
  L.arrays = at; at += 11 * up16((size_t)cap * 4);
  L.edge_sums = at; at += up16((size_t)L.edge_blocks * 4);
  L.edge_offs = at; at += up16((size_t)L.edge_blocks * 4);
  L.end = at;
  return L;
}

#define LAUNCH(kernel, grid, block, ...)                              \
  do {                                                                \
    hipLaunchKernelGGL(kernel, dim3((unsigned)(grid)), dim3(block), 0, st, __VA_ARGS__); \
    const int32_t rc_ = unet_check_launch(#kernel);                   \
    if (rc_) return rc_;                                              \
  } while (0)

// the counting stage: code, offs (of the edges) and counts
int32_t count_stage(const Frames& A, const Layout& L, char* ws, long long* counts, hipStream_t st) {
  unsigned short* code = (unsigned short*)(ws + L.code);
  int* sums = (int*)(ws + L.sums);
  int* offs = (int*)(ws + L.offs);
  long long* totals = (long long*)(ws + L.totals);
  const int blocks = (int)L.blocks;
  LAUNCH(mark_edges, blocks, THREADS, A, code, sums, blocks);
  for (int f = 0; f < 4; ++f)
    LAUNCH(scan_spine, 1, SPINE_THREADS, sums + (size_t)f * blocks, offs + (size_t)f * blocks, blocks,
           cdiv(blocks, SPINE_THREADS), totals + f);
  LAUNCH(finish_counts, 1, WAVE, totals, counts);
  return UNET_OK;
}

// out = the exclusive prefix sums of the live entries of in (in == out is fine)
int32_t scan_edges(const long long* counts, int64_t cap, const Layout& L, char* ws, const int* in, int* out, hipStream_t st) {
  int* sums = (int*)(ws + L.edge_sums);
  int* offs = (int*)(ws + L.edge_offs);
  const int blocks = (int)L.edge_blocks;
  LAUNCH(scan_sums, blocks, THREADS, counts, (long long)cap, in, sums);
  LAUNCH(scan_spine, 1, SPINE_THREADS, (const int*)sums, offs, blocks, cdiv(blocks, SPINE_THREADS), (long long*)nullptr);
  LAUNCH(scan_apply, blocks, THREADS, counts, (long long)cap, in, (const int*)offs, out);
  return UNET_OK;
}

int32_t check_frames(const char* who, const void* region, const void* sizes, const void* counts, const void* workspace,
                     int64_t n, int64_t h, int64_t w, int32_t min_pixels) {
  UNET_REQUIRE(region && sizes && counts && workspace, UNET_ERR_BAD_ARG, "%s: null pointer", who);
  UNET_REQUIRE(n > 0 && h > 0 && w > 0 && min_pixels >= 1, UNET_ERR_BAD_ARG, "%s: n=%lld h=%lld w=%lld min_pixels=%d", who,
               (long long)n, (long long)h, (long long)w, (int)min_pixels);
  UNET_REQUIRE(supported(n, h, w), UNET_ERR_UNSUPPORTED, "%s: n=%lld h=%lld w=%lld (n < 65536, at most 2^29 pixels)", who,
               (long long)n, (long long)h, (long long)w);
  return UNET_OK;
}

}  // namespace

extern "C" size_t unet_count_class_region_edges_workspace(int64_t n, int64_t h, int64_t w) {
  if (!supported(n, h, w)) return 0;
  return layout(n, h, w, 0).end_count;
}

extern "C" int32_t unet_count_class_region_edges(const int32_t* region, const int32_t* sizes, int64_t n, int64_t h,
                                                 int64_t w, int32_t min_pixels, int64_t* counts, void* workspace,
                                                 size_t workspace_bytes, void* stream) {
  const char* who = "unet_count_class_region_edges";
  const int32_t rc = check_frames(who, region, sizes, counts, workspace, n, h, w, min_pixels);
  if (rc) return rc;
  UNET_REQUIRE(workspace_bytes >= unet_count_class_region_edges_workspace(n, h, w), UNET_ERR_WORKSPACE,
               "%s: workspace too small", who);
  const Frames A{region, sizes, (int)min_pixels, 0, (int)h, (int)w, (long long)(h * w), (long long)(n * h * w)};
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(UNET_K_OTHER, 0.0, st, "mark_edges", (double)n * h * w * 10.0);
  return count_stage(A, layout(n, h, w, 0), (char*)workspace, (long long*)counts, st);
}

extern "C" size_t unet_trace_class_regions_workspace(int64_t n, int64_t h, int64_t w, int64_t edge_cap) {
  if (!supported(n, h, w) || edge_cap < 0 || edge_cap > (1LL << 31) - 1) return 0;
  return layout(n, h, w, edge_cap).end;
}

extern "C" int32_t unet_trace_class_regions(const int32_t* region, const int32_t* sizes, int64_t n, int64_t h, int64_t w,
                                            int32_t min_pixels, int32_t image_base, int64_t edge_cap, int64_t* loops,
                                            int64_t loop_cap, int32_t* points, int64_t point_cap, int64_t* counts,
                                            void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "unet_trace_class_regions";
  const int32_t rc = check_frames(who, region, sizes, counts, workspace, n, h, w, min_pixels);
  if (rc) return rc;
  UNET_REQUIRE((loops || loop_cap == 0) && (points || point_cap == 0), UNET_ERR_BAD_ARG, "%s: null pointer", who);
  UNET_REQUIRE(image_base >= 0 && edge_cap >= 0 && loop_cap >= 0 && point_cap >= 0, UNET_ERR_BAD_ARG,
               "%s: image_base=%d edge_cap=%lld loop_cap=%lld point_cap=%lld", who, (int)image_base, (long long)edge_cap,
               (long long)loop_cap, (long long)point_cap);
  const int64_t lim = (1LL << 31) - 1;
  UNET_REQUIRE((int64_t)image_base + n <= lim && edge_cap <= lim && loop_cap <= lim && point_cap <= lim,
               UNET_ERR_UNSUPPORTED, "%s: image_base=%d edge_cap=%lld loop_cap=%lld point_cap=%lld (all below 2^31)", who,
               (int)image_base, (long long)edge_cap, (long long)loop_cap, (long long)point_cap);
  UNET_REQUIRE(workspace_bytes >= unet_trace_class_regions_workspace(n, h, w, edge_cap), UNET_ERR_WORKSPACE,
               "%s: workspace too small", who);
  const Frames A{region, sizes, (int)min_pixels, (int)image_base, (int)h, (int)w, (long long)(h * w), (long long)(n * h * w)};
  const Layout L = layout(n, h, w, edge_cap);
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(UNET_K_OTHER, 0.0, st, "trace_class_regions", (double)n * h * w * 10.0 + (double)edge_cap * 44.0);
  int32_t rc2 = count_stage(A, L, ws, (long long*)counts, st);
  if (rc2 || edge_cap == 0) return rc2;

  const size_t stride = up16((size_t)edge_cap * 4);
  int* arr[11];
  for (int i = 0; i < 11; ++i) arr[i] = (int*)(ws + L.arrays + (size_t)i * stride);
  const long long* cnt = (const long long*)counts;
  const Edges E{(const unsigned short*)(ws + L.code), (const int*)(ws + L.offs), cnt, (long long)edge_cap,
                arr[0], arr[1], arr[2]};
  int* next[2] = {arr[3], arr[4]};                     // after the leaders are known: the cut predecessor pointers
  int* low[2] = {arr[5], arr[6]};
  int* rank[2] = {arr[7], arr[8]};
  int* loop_index = arr[9];
  int* first_point = arr[10];
  int rounds = 0;                                      // 2^rounds >= the longest loop there can be
  while ((1LL << rounds) < edge_cap) ++rounds;
  const unsigned per_edge = (unsigned)cdiv64(edge_cap, THREADS);

  LAUNCH(link_edges, L.blocks, THREADS, A, E, next[0], low[0]);
  for (int r = 0; r < rounds; ++r)
    LAUNCH(double_min, per_edge, THREADS, cnt, (long long)edge_cap, (const int*)next[r & 1], (const int*)low[r & 1],
           next[(r + 1) & 1], low[(r + 1) & 1]);
  const int* leader = low[rounds & 1];
  int* n_points = low[(rounds + 1) & 1];               // the other minimum buffer is free now
  LAUNCH(start_ranks, per_edge, THREADS, E, leader, next[0], rank[0], loop_index);
  for (int r = 0; r < rounds; ++r)
    LAUNCH(double_sum, per_edge, THREADS, cnt, (long long)edge_cap, (const int*)next[r & 1], (const int*)rank[r & 1],
           next[(r + 1) & 1], rank[(r + 1) & 1]);
  const int* ranks = rank[rounds & 1];
  LAUNCH(loop_points, per_edge, THREADS, E, leader, ranks, n_points);
  if ((rc2 = scan_edges(cnt, edge_cap, L, ws, loop_index, loop_index, st))) return rc2;
  if ((rc2 = scan_edges(cnt, edge_cap, L, ws, n_points, first_point, st))) return rc2;
  const Rows R{leader, ranks, loop_index, first_point, n_points, (long long*)loops, (long long)loop_cap, (int*)points,
               (long long)point_cap};
  LAUNCH(write_rows, per_edge, THREADS, A, E, R);
  LAUNCH(emit_points, per_edge, THREADS, A, E, R);
  return UNET_OK;
}
