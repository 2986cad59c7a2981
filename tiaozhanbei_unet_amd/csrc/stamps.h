// The stamp clock of the diagnostic build (`make stamps`, -DPDMA_STAMPS; read by tools/stamps.py): per-wave sums of
// s_memtime differences over the phases ("laps") of a kernel's main loop.  The stamped kernels (conv3_pdma_body,
// conv3_ws16_kernel, wgrad_dma_kernel, wgrad16_kernel) call the clock unconditionally: in the default build StampClock
// is an empty struct whose methods do nothing, so no stamp executes there and the device code is that of a source
// without them.  Apart from the stamps-only members of the parameter structs, their assignment in the launchers and the
// setter, this header is the only place that names PDMA_STAMPS.
//
// One record per wave, eight uint64: laps [0..5], count [6] (taps or tiles), clock [7] = (d memtime << 20) /
// (d memrealtime + 1), i.e. the shader clock in units of the 100 MHz reference, x 2^20.  Lane 0 of each wave writes
// record blockIdx.x * waves_per_block + wave with plain stores, and only if that index is below the capacity that came
// with the pointer (unet_debug_set_buffer): a block beyond the buffer writes nothing.
//
// Stamps cost about 10 % themselves and their fences forbid overlaps the real kernel has: read a stamped build's
// SHARES, never its run time.  Open remark: a builtin-form stamp is followed by the compiler's own lgkmcnt(0), which
// inside a section with hand-counted lgkmcnt(N) waits drains LDS reads the real kernel leaves in flight; the sites are
// where they were measured (profiles/), moving or re-fencing them is a decision of its own.
#pragma once

#ifdef PDMA_STAMPS
struct StampSink { unsigned long long* p; long long records; };   // device buffer of `records` 8-word records
#define STAMP_SINK(member_expr) (member_expr)
extern StampSink g_stamp_sink;     // set by unet_debug_set_buffer (conv_api.hip), copied into the params by the launchers

struct StampClock {
  unsigned long long lap[6], prev, n, t0, r0;
  __device__ __forceinline__ unsigned long long now() const { return __builtin_amdgcn_s_memtime(); }
  // running = false: the first lap opens at the first resume(), not here
  __device__ __forceinline__ void start(bool running = true) {
    for (int i = 0; i < 6; ++i) lap[i] = 0;
    n = 0;
    t0 = __builtin_amdgcn_s_memtime();
    r0 = __builtin_amdgcn_s_memrealtime();
    prev = running ? t0 : 0;
  }
  __device__ __forceinline__ unsigned long long last() const { return prev; }
  __device__ __forceinline__ void add(int i, unsigned long long cycles) { lap[i] += cycles; }
  // now - previous stamp -> lap i.  FENCED: __builtin_amdgcn_sched_barrier(0) before and after the stamp
  // (conv3_ws16_kernel's form; the other kernels place their fences themselves)
  template <bool FENCED = false>
  __device__ __forceinline__ void mark(int i) {
    if (FENCED) __builtin_amdgcn_sched_barrier(0);
    const unsigned long long t = now();
    lap[i] += t - prev;
    prev = t;
    if (FENCED) __builtin_amdgcn_sched_barrier(0);
  }
  __device__ __forceinline__ void resume(int i) {          // mark(i) unless paused; the next lap opens here either way
    const unsigned long long t = now();
    if (prev) lap[i] += t - prev;
    prev = t;
  }
  __device__ __forceinline__ void pause() { prev = 0; }
  __device__ __forceinline__ void tick() { n += 1; }       // a count kept by the clock (taps), for store()
  __device__ __forceinline__ unsigned long long ticks() const { return n; }
  __device__ __forceinline__ void store(StampSink sink, int waves_per_block, unsigned long long count) const {
    const long long rec = (long long)blockIdx.x * waves_per_block + (threadIdx.x >> 6);
    if (sink.p && (threadIdx.x & 63) == 0 && rec < sink.records) {
      unsigned long long* o = sink.p + rec * 8;
      for (int i = 0; i < 6; ++i) o[i] = lap[i];
      o[6] = count;
      o[7] = ((__builtin_amdgcn_s_memtime() - t0) << 20) / (__builtin_amdgcn_s_memrealtime() - r0 + 1);
    }
  }
};
#else
struct StampSink {};
#define STAMP_SINK(member_expr) (StampSink{})              // the member exists in the diagnostic build only

struct StampClock {
  __device__ __forceinline__ unsigned long long now() const { return 0; }
  __device__ __forceinline__ void start(bool = true) {}
  __device__ __forceinline__ unsigned long long last() const { return 0; }
  __device__ __forceinline__ void add(int, unsigned long long) {}
  template <bool FENCED = false>
  __device__ __forceinline__ void mark(int) {}
  __device__ __forceinline__ void resume(int) {}
  __device__ __forceinline__ void pause() {}
  __device__ __forceinline__ void tick() {}
  __device__ __forceinline__ unsigned long long ticks() const { return 0; }
  __device__ __forceinline__ void store(StampSink, int, unsigned long long) const {}
};
#endif
