// trace_rays.hip — bdpt_trace_rays: closest-hit and any-hit queries on a caller's rays in device memory.
//
// Replaces TraceRay from a caller's own ray-generation shader (CommonPasses/Data/CommonPasses/aoTracing.rt.hlsl:112,
// lambertianPlusShadows.rt.hlsl:62, simpleDiffuseGI.rt.hlsl:127, BDPT/standardShadowRay.hlsli:40).  The query modes are
// those of device_trace.hpp (and of oracle_trace): 0 closest hit, 1 closest hit with back faces culled, 2 any hit.
//
// One persistent kernel per mode, built as trace_shadow_kernel is (device_trace.hpp): one wave per workgroup, 64
// traversal slots per wave refilled from the ray list by ballot + popcount prefix with one atomic per chunk, while-while
// traversal with deferred leaves, kStackLds stack rows in LDS and the rest in the context's overflow area.  What differs:
// closest-hit modes enter children nearest first; tmin is per ray; a ray is two float4 loads, a hit one float4 store;
// the list is one dense array whose length may be a device word.
#include "kernels.h"

#include "device_math.hpp"
#include "device_query.hpp"
#include "device_scene.hpp"
#include "device_trace.hpp"
#include "launch.hpp"

namespace bdpt {

// rays[2i] = (org, tmin), rays[2i+1] = (dir, tmax) (bdpt_ray); hits[i] = (t, u, v, prim bits) (bdpt_hit); vis[i] = 1 unoccluded.
// cursor[0]: next ray to hand out, cursor[1]: waves done; both zero when a launch starts and when it ends.
template <int MODE>
__global__ __launch_bounds__(kWave) void trace_rays_kernel(SceneDev S, const float4* __restrict__ rays, uint32_t cap,
                                                           const uint32_t* count, unsigned long long* cursor,
                                                           float4* __restrict__ hits, uint8_t* __restrict__ vis) {
  BDPT_ONE_WAVE_PER_GROUP();
  __shared__ int s_stack[kStackLds * kWave];
  int* stk = s_stack + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const uint32_t n = itemCount(cap, count);
  // rays per atomic: up to kFetchChunk, no more than a fair share per wave (a short list still spreads over the grid)
  const uint32_t share = (n / gridDim.x + kWave - 1) & ~(uint32_t)(kWave - 1);
  const uint32_t chunk = share < (uint32_t)kWave ? (uint32_t)kWave : (share > kFetchChunk ? kFetchChunk : share);
  bool has = false, exhausted = false;
  uint32_t rid = 0, chunkPos = 0, chunkEnd = 0;
  uint32_t nTris = 0, nAlpha = 0;  // (leafStep's tallies: not kept)
  TravState T;
  T.cur = kDone;
  for (;;) {
    const unsigned long long idleMask = __ballot(!has);
    const int idle = __popcll(idleMask);
    if (!exhausted && idle >= kRefillIdle) {
      if (chunkPos >= chunkEnd) {  // wave-uniform: take a new chunk
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(cursor, (unsigned long long)chunk);
        base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(base >> 32)) << 32) |
               (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
        if (base < n) {
          chunkPos = (uint32_t)base;
          chunkEnd = (base + chunk < n) ? (uint32_t)(base + chunk) : n;
        } else {
          exhausted = true;
        }
      }
      if (!exhausted) {
        const uint32_t avail = chunkEnd - chunkPos;
        const uint32_t take = ((uint32_t)idle < avail) ? (uint32_t)idle : avail;
        const uint32_t rank = (uint32_t)__popcll(idleMask & ((1ull << lane) - 1ull));
        if (!has && rank < take) {
          rid = chunkPos + rank;
          const float4 a = rays[(size_t)rid * 2], b = rays[(size_t)rid * 2 + 1];
          travInit(T, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), a.w, b.w);
          has = true;
        }
        chunkPos += take;
      }
    }
    if (__ballot(has) == 0ull) break;  // exhausted and every lane retired
#if BDPT_LEAF_WAIT > 0
    // deferred leaves, as trace_shadow_kernel: node bursts; leaves once BDPT_LEAF_WAIT_FRAC8 eighths of the lanes wait at one
    {
      uint32_t nNodes = 0;
      int maxSp = 0;
      nodeBurst<(MODE != 2) ? 1 : 0, kStackLds, BDPT_NODE_BURST, false>(S, T, stk, has, nNodes, maxSp);
    }
    const unsigned long long waitMask = __ballot(has && T.cur < 0), nodeMask = __ballot(has && T.cur >= 0);
    const int waitNeed = (__popcll(waitMask | nodeMask) * BDPT_LEAF_WAIT_FRAC8 + 7) >> 3;
    const bool leafPhase = (int)__popcll(waitMask) >= waitNeed || nodeMask == 0ull;
#else
    if (has)
      while (T.cur >= 0) nodeStep<(MODE != 2) ? 1 : 0, kStackLds>(S, T, stk);
    const bool leafPhase = true;
#endif
    if (leafPhase && has && T.cur < 0) {
      bool finished = (T.cur == kDone);
      if (!finished) {
        finished = leafStep<MODE, false>(S, T, nTris, nAlpha);
        if (!finished) {
          T.cur = travPop<kStackLds>(S, T, stk);
          finished = (T.cur == kDone);
        }
      }
      if (finished) {
        if (MODE == 2) {
          vis[rid] = (T.best.prim < 0) ? (uint8_t)1 : (uint8_t)0;
        } else {
          const bool hit = T.best.prim >= 0;
          hits[rid] = make_float4(hit ? T.best.t : 0.0f, hit ? T.best.u : 0.0f, hit ? T.best.v : 0.0f, __int_as_float(T.best.prim));
        }
        has = false;
        T.cur = kDone;
      }
    }
  }
  // The last wave to finish leaves the cursor at zero for the next launch, so a call (and a graph made of it) is this one
  // kernel: every other wave has taken its last chunk before it counts itself done.
  if (lane == 0) {
    __threadfence();
    if (atomicAdd(&cursor[1], 1ull) == (unsigned long long)gridDim.x - 1ull) {
      cursor[0] = 0ull;
      cursor[1] = 0ull;
    }
  }
}

void launchTraceRays(const SceneDev& S, const float4* rays, uint32_t cap, const uint32_t* count, unsigned long long* cursor, int mode,
                     float4* hits, uint8_t* vis, LaunchGrids& G, int numCUs, hipStream_t st) {
  if (!cap) return;
  static constexpr decltype(&trace_rays_kernel<0>) kByMode[3] = {trace_rays_kernel<0>, trace_rays_kernel<1>, trace_rays_kernel<2>};
  const auto kernel = kByMode[mode];
  uint32_t& g = G.rays[mode];
  if (!g) g = persistentGrid(kernel, numCUs);
  const uint32_t need = wavesFor(cap);
  launchWave(kernel, g < need ? g : need, st, S, rays, cap, count, cursor, hits, vis);
}

}  // namespace bdpt
