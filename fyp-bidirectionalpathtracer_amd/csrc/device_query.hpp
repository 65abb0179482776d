// device_query.hpp — what the per-item query kernels share (trace_rays.hip, surface_query.hip, light_query.hip,
// connect_query.hip, motion.hip): the item count of a launch, a lane's place in it, and the compacted ray list.
// QueryRange and CompactList, which the host fills, are in kernels.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace bdpt {

// The number of items a launch covers: min(*count, cap), or cap without a device word (wave-uniform).
__device__ __forceinline__ uint32_t itemCount(uint32_t cap, const uint32_t* count) {
  if (!count) return cap;
  const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)*count);
  return c < cap ? c : cap;
}

// The prologue of a lane on a dense grid of one-wave workgroups, one lane per item: sets the lane's item i and the item
// count n, and returns true when the lane has nothing left to do and returns.  That is its own i >= n, except in a COMPACT
// instance, where it is wave-uniform (the wave is wholly past the count) and a lane with i >= n stays for the wave's ballot.
template <bool COMPACT = false>
__device__ __forceinline__ bool queryLanePast(uint32_t cap, const uint32_t* count, uint32_t& i, uint32_t& n) {
  i = blockIdx.x * kWave + threadIdx.x;
  n = itemCount(cap, count);
  return COMPACT ? (blockIdx.x * kWave >= n) : (i >= n);
}
__device__ __forceinline__ bool queryLanePast(uint32_t cap, const uint32_t* count, uint32_t& i) {
  uint32_t n;
  return queryLanePast(cap, count, i, n);
}

// Appends the rays (q0, q1) of the lanes with `emit` to the list, with their item indices: one ballot + popcount prefix
// and one atomic per wave, as emitRay appends to the pass's ray queue.  Every lane of the wave calls it.
__device__ __forceinline__ void compactAppend(const CompactList& list, uint32_t cap, bool emit, uint32_t i, float4 q0, float4 q1) {
  const unsigned long long mask = __ballot(emit);
  if (mask == 0ull) return;
  const int lane = (int)(threadIdx.x & 63u);
  const int leader = __ffsll((long long)mask) - 1;
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(list.count, (uint32_t)__popcll(mask));
  base = (uint32_t)__shfl((int)base, leader);
  const uint32_t at = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
  if (emit && at < cap) {  // (at < cap always when the caller zeroed the word: never write past the lists)
    list.rays[(size_t)at * 2] = q0;
    list.rays[(size_t)at * 2 + 1] = q1;
    list.items[at] = i;
  }
}

}  // namespace bdpt
