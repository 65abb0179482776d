// launch.hpp — host-side launch helpers of the one-wave-per-workgroup kernels (every .hip file but bvh_device.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "kernels.h"

namespace bdpt {

#ifndef PERCU
#define PERCU 24
#endif

// one-wave workgroups that cover n lanes
static inline uint32_t wavesFor(uint64_t n) { return (uint32_t)((n + kWave - 1) / kWave); }

// fn(std::true_type{}) or fn(std::false_type{}): a run-time switch as a template argument of the kernel
template <class Fn>
static void withFlag(bool f, Fn&& fn) {
  if (f)
    fn(std::true_type{});
  else
    fn(std::false_type{});
}

// ONE WORKGROUP = ONE WAVE (kernels.hip, above its launchers, lists what relies on it).  The kernels declared
// __launch_bounds__(kWave) are launched through launchWave() only — there is no block size to get wrong — and each
// starts with BDPT_ONE_WAVE_PER_GROUP(), which makes a launch of any other shape do nothing instead of corrupting.
template <class K, class... Args>
static void launchWave(K kernel, uint32_t grid, hipStream_t st, Args... args) {
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kWave), 0, st, args...);
}

// the same with `ldsBytes` of dynamic LDS (extern __shared__)
template <class K, class... Args>
static void launchWaveLds(K kernel, uint32_t grid, size_t ldsBytes, hipStream_t st, Args... args) {
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kWave), ldsBytes, st, args...);
}

// Persistent grids: as many one-wave workgroups as can be resident (LDS 8 KiB/wave, VGPRs).
template <class K>
static uint32_t persistentGrid(K kernel, int numCUs) {
  int perCU = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, kWave, 0) != hipSuccess || perCU <= 0) perCU = 8;
  if (perCU > PERCU) perCU = PERCU;
  if (perCU > kMaxPersistentPerCU) perCU = kMaxPersistentPerCU;  // the stack overflow area is sized for that many
  return (uint32_t)(perCU * numCUs);
}

// A persistent kernel over a list of up to `cap` items: its resident grid (asked once per kernel and kept in the
// context's `gridSlot`, a LaunchGrids word), no larger than the waves the items can fill.
template <class K, class... Args>
static void launchPersistent(K kernel, uint32_t& gridSlot, uint32_t cap, int numCUs, hipStream_t st, Args... args) {
  if (!gridSlot) gridSlot = persistentGrid(kernel, numCUs);
  const uint32_t need = wavesFor(cap);
  launchWave(kernel, gridSlot < need ? gridSlot : need, st, args...);
}

}  // namespace bdpt
