// sky.hip — bdpt_sky_query and bdpt_sky_execute: sky lighting, S importance-sampled any-hit rays per item toward the
// environment map, from one persistent kernel.
//
// Replaces the loop a caller otherwise runs per sample: bdpt_env_query(SAMPLE, matIndex 1) -> clamp -> glue that keeps the
// non-zero terms -> bdpt_trace_rays(BDPT_TRACE_ANY) -> an ordered add (include/bdpt.h "Environment lighting" has the
// definition; the two are equal bit for bit).
//
// Built on the item loop of device_item_loop.hpp (refill, nodePhase, leafPhase, releaseCursor), shaped like ao_kernel: a
// lane owns its item through all its samples.  When its ray is answered it adds the term, draws its next direction from
// the table (envSample of env_light.h: two binary searches, in its own slot) and starts that ray; samples whose value is
// all +-0 trace no ray and are passed over at once.  After sample S-1 the lane retires with one store per output: no output
// atomics, every word has one writer, whatever the order the lanes run in.  Dead items never take a slot: their outputs
// are written at fetch.  Across the traversal a lane keeps its item, k, count, the RNG state, the sum and the term its
// ray gates; N and diffuse are re-read from the record when it regenerates, the origin lives in the traversal state.
// The item itself, a record or a G-buffer pixel, is read and written through device_item_source.hpp.
#include "kernels.h"

#include "device_item_loop.hpp"
#include "device_item_source.hpp"
#include "device_math.hpp"
#include "device_query.hpp"
#include "device_scene.hpp"
#include "env_light.h"
#include "launch.hpp"

namespace bdpt {

// Waves per SIMD the register allocation aims for (experiment knob, as BDPT_AO_WAVES_PER_EU of ao.hip): DESIGN.md
// "Environment lighting" has the resource usage of both instances.
#ifndef BDPT_SKY_WAVES_PER_EU
#define BDPT_SKY_WAVES_PER_EU 4
#endif

namespace {

// the outputs of item `i`
template <int SRC>
__device__ __forceinline__ void skyStore(const SkyDev& Q, uint32_t i, f3 color, uint32_t count, uint32_t seed) {
  itemStoreColor<SRC>(Q, i, color);
  if (SRC == ITEM_SRC_SURFACES) {
    if (Q.counts) Q.counts[i] = count;
    if (Q.seedsOut) Q.seedsOut[i] = seed;
  }
}

// The item's samples from k on, in order: a sample whose clamped value is all +-0 is added at once (no ray); the first
// other one starts its ray from `pos` and is kept in `pend`.  Returns whether a ray is in flight; false: k == samples.
template <int SRC>
__device__ __forceinline__ bool skyNext(const SkyDev& Q, uint32_t i, f3 pos, uint32_t& k, uint32_t& seed, f3& sum, f3& pend, TravState& T) {
  const f3 N = itemNormal<SRC>(Q, i), dif = itemDiffuse<SRC>(Q, i);
  while (k < Q.samples) {
    k++;
    const EnvSample e = envSample(Q.table, seed);
    const f3 dir = mk(e.dir[0], e.dir[1], e.dir[2]);
    f3 value = mk(0);
    if (e.pdf != 0.0f) {
      const float NdotL = saturate(dot(N, dir));
      value = clampVec((((NdotL * mk(e.radiance[0], e.radiance[1], e.radiance[2])) * dif) / kPi) / e.pdf, Q.clampUpper);
    }
    if (allZero(value)) {
      sum = sum + value;
      continue;
    }
    pend = value;
    travInit(T, pos, dir, Q.range.minT, 1e+38f);
    return true;
  }
  return false;
}

}  // namespace

// cursor: as releaseCursor has it (both words zero when a launch starts and when it ends).
template <int SRC>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(BDPT_SKY_WAVES_PER_EU, 8))) void sky_kernel(
    SceneDev S, SkyDev Q, unsigned long long* cursor) {
  BDPT_ONE_WAVE_PER_GROUP();
  __shared__ int s_stack[kStackLds * kWave];
  int* stk = s_stack + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  ItemFeed F = feedInit(itemCount(Q.range.cap, Q.range.count));
  bool has = false;
  uint32_t rid = 0, k = 0, count = 0, seed = 0;
  f3 sum = mk(0), pend = mk(0);
  TravState T;
  T.cur = kDone;
  while (refill(F, cursor, lane, has, [&](uint32_t item) {
    rid = item;
    seed = itemSeed<SRC>(Q, rid);
    f3 pos = mk(0);
    if (!itemAlive<SRC>(Q, rid, pos)) {
      skyStore<SRC>(Q, rid, itemDiffuse<SRC>(Q, rid), 0u, seed);  // the background: the diffuse channel holds the colour, no draw; the lane stays idle
    } else {
      k = 0;
      count = 0;
      sum = mk(0);
      if (skyNext<SRC>(Q, rid, pos, k, seed, sum, pend, T)) {
        has = true;
      } else {
        skyStore<SRC>(Q, rid, sum / (float)Q.samples, 0u, seed);  // no sample of the item was worth a ray
      }
    }
  })) {
    const bool leavesDue = nodePhase<0>(S, T, stk, has);
    if (leavesDue && has && T.cur < 0 && leafPhase<BDPT_TRACE_ANY>(S, T, stk)) {
      if (T.best.prim < 0) {  // unoccluded
        sum = sum + pend;
        count++;
      }
      if (!skyNext<SRC>(Q, rid, T.o, k, seed, sum, pend, T)) {
        skyStore<SRC>(Q, rid, sum / (float)Q.samples, count, seed);
        has = false;
        T.cur = kDone;
      }
    }
  }
  releaseCursor(cursor, lane);
}

void launchSky(const SceneDev& S, const SkyDev& Q, bool gbuffer, unsigned long long* cursor, LaunchGrids& G, int numCUs, hipStream_t st) {
  if (!Q.range.cap) return;
  withFlag(gbuffer, [&](auto GB) {
    launchPersistent(sky_kernel<GB ? ITEM_SRC_GBUFFER : ITEM_SRC_SURFACES>, G.sky[GB ? 1 : 0], Q.range.cap, numCUs, st, S, Q, cursor);
  });
}

}  // namespace bdpt
