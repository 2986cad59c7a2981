// The accumulator tail of the region describers (defects.hip: where a region lies and how sure the model was; shapes.hip:
// moments, bit quads, projections).  Both make one record per kept region of unet_label_class_regions in two launches
// over the pixels, blocks of PX_THREADS: an assign pass gives every kept root pixel a slot in the record buffer and
// leaves it in a per-pixel workspace, an accumulate pass folds every other pixel into the record of its region's slot.
//   flush_by_slot   the end of the accumulate pass.  Each thread arrives with what its pixels of one slot add up to (the
//                   caller folds a thread's pixels while the slot stays the same and commits when it changes).  The wave
//                   reduces the lanes that share the slot of its first pending lane with shuffles, LEADERS times over;
//                   the lanes that remain commit on their own.  The first such sum of each of the block's waves goes
//                   through LDS, where one thread folds the waves that share a slot.  A region that fills the frame costs
//                   one commit per block; a wave of many small regions falls back to per-lane commits.
//   wave_slot       a slot in a record buffer for every lane that has a record to append (segregions.hip's region
//                   records, groups.hip's fragment records): one atomicAdd per wave on the device-side count.
// What the caller brings: a struct Acc with an int `slot` (< 0: nothing) and, in the namespace of Acc (the including
// file's unnamed one: flush_by_slot calls them unqualified and argument-dependent lookup finds them there),
// fold(Acc&, const Acc&) and wave_fold(Acc, bool on) -> the fold over the lanes with `on` (every lane calls it); and a
// commit functor that adds an Acc to its record with atomics.  All sums are integers: exact in any order.
// The assign pass stays written out in both files: every shared form changed its device code (profiles/shared_bodies.txt).
#pragma once
#include "unionfind.h"

namespace slots {

constexpr int LEADERS = 4;                             // slots per wave that are reduced with shuffles
constexpr int PX_WAVES = uf::PX_THREADS / WAVE;

// slot of every lane that is on in the record buffer counted by *counter: one atomicAdd per wave
__device__ __forceinline__ long long wave_slot(unsigned long long* counter, bool on, int lane) {
  const unsigned long long m = __ballot(on);
  if (!m) return -1;                                   // wave-uniform
  const int first = __ffsll((long long)m) - 1;
  unsigned long long at = 0;
  if (lane == first) at = atomicAdd(counter, (unsigned long long)__popcll(m));
  at = __shfl(at, first);
  return on ? (long long)(at + __popcll(m & ((1ull << lane) - 1ull))) : -1;
}

// a: what the thread still holds (a.slot < 0: nothing).  Every thread of the block calls this, at the kernel's end.
template <class Acc, class Commit>
__device__ __forceinline__ void flush_by_slot(Acc a, Commit commit) {
  __shared__ Acc part[PX_WAVES];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  // the wave: the lanes that share the slot of the first pending lane are summed with shuffles, LEADERS times over
  Acc mine;
  mine.slot = -1;
  unsigned long long m = __ballot(a.slot >= 0);
  for (int it = 0; it < LEADERS && m; ++it) {          // wave-uniform
    const int first = __ffsll((long long)m) - 1;
    const int lead = __shfl(a.slot, first);
    const bool on = a.slot == lead;
    const unsigned long long same = __ballot(on);
    Acc s = wave_fold(a, on);
    s.slot = lead;
    if (it == 0) mine = s;
    else if (lane == first) commit(s);
    if (on) a.slot = -1;
    m &= ~same;
  }
  if (a.slot >= 0) commit(a);                          // a wave of more than LEADERS regions: each lane for itself
  // the block: the waves' first sums, folded where they share a slot
  if (lane == 0) part[wave] = mine;
  __syncthreads();
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int i = 0; i < PX_WAVES; ++i) {
    Acc s = part[i];
    if (s.slot < 0) continue;
#pragma unroll
    for (int j = i + 1; j < PX_WAVES; ++j)
      if (part[j].slot == s.slot) { fold(s, part[j]); part[j].slot = -1; }
    commit(s);
  }
}

}  // namespace slots
