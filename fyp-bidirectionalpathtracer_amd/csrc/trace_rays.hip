// trace_rays.hip — bdpt_trace_rays: closest-hit and any-hit queries on a caller's rays in device memory.
//
// Replaces TraceRay from a caller's own ray-generation shader (CommonPasses/Data/CommonPasses/aoTracing.rt.hlsl:112,
// lambertianPlusShadows.rt.hlsl:62, simpleDiffuseGI.rt.hlsl:127, BDPT/standardShadowRay.hlsli:40).  The query modes are
// those of device_trace.hpp (and of oracle_trace): 0 closest hit, 1 closest hit with back faces culled, 2 any hit.
//
// One persistent kernel per mode on the item loop of device_item_loop.hpp (fetch, node and leaf phases, cursor release).
// What is its own: closest-hit modes enter children nearest first; tmin is per ray; a ray is two float4 loads, a hit one
// float4 store; the list is one dense array whose length may be a device word.
#include "kernels.h"

#include "device_item_loop.hpp"
#include "device_math.hpp"
#include "device_query.hpp"
#include "device_scene.hpp"
#include "launch.hpp"

namespace bdpt {

// rays[2i] = (org, tmin), rays[2i+1] = (dir, tmax) (bdpt_ray); hits[i] = (t, u, v, prim bits) (bdpt_hit); vis[i] = 1 unoccluded.
// cursor: the context's two words (releaseCursor), both zero when a launch starts and when it ends.
template <int MODE>
__global__ __launch_bounds__(kWave) void trace_rays_kernel(SceneDev S, const float4* __restrict__ rays, uint32_t cap,
                                                           const uint32_t* count, unsigned long long* cursor,
                                                           float4* __restrict__ hits, uint8_t* __restrict__ vis) {
  BDPT_ONE_WAVE_PER_GROUP();
  __shared__ int s_stack[kStackLds * kWave];
  int* stk = s_stack + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  ItemFeed F = feedInit(itemCount(cap, count));
  bool has = false;
  uint32_t rid = 0;
  TravState T;
  T.cur = kDone;
  while (refill(F, cursor, lane, has, [&](uint32_t item) {
    rid = item;
    const float4 a = rays[(size_t)rid * 2], b = rays[(size_t)rid * 2 + 1];
    travInit(T, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), a.w, b.w);
    has = true;
  })) {
    const bool leavesDue = nodePhase<(MODE != 2) ? 1 : 0>(S, T, stk, has);
    if (leavesDue && has && T.cur < 0 && leafPhase<MODE>(S, T, stk)) {
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
  releaseCursor(cursor, lane);
}

void launchTraceRays(const SceneDev& S, const float4* rays, uint32_t cap, const uint32_t* count, unsigned long long* cursor, int mode,
                     float4* hits, uint8_t* vis, LaunchGrids& G, int numCUs, hipStream_t st) {
  if (!cap) return;
  static constexpr decltype(&trace_rays_kernel<0>) kByMode[3] = {trace_rays_kernel<0>, trace_rays_kernel<1>, trace_rays_kernel<2>};
  launchPersistent(kByMode[mode], G.rays[mode], cap, numCUs, st, S, rays, cap, count, cursor, hits, vis);
}

}  // namespace bdpt
