// walk_query.hip — bdpt_walk_query: whole subpaths of a caller's integrator from one persistent kernel.
//
// Replaces the loop a caller otherwise runs per bounce on the host — bdpt_trace_rays(CLOSEST), bdpt_shade_hits,
// bdpt_bsdf_query(SAMPLE) and glue that selects the hits, multiplies the colours and builds the next rays — i.e. shootRay /
// the closest-hit shader of the reference's walks (BDPT/BDPTMain.rt.hlsl:106-145, BDPT/globalIlluminationRay.hlsli:1-45).
//
// Built on the item loop of device_item_loop.hpp (fetch, node and leaf phases, parking, cursor release) with closest-hit
// rays.  What is its own is what an answered lane does: it shades the hit (shadeHit<false>, seen from the ray's origin,
// as shade_hits_kernel), samples the record (sampleBRDF on the stored words, as bsdf_query_kernel), writes vertex `step`
// and, while steps remain, starts the next ray in its own slot; it retires when its walk has ended, after writing the
// steps that do not exist.  Finished lanes wait until BDPT_WALKQ_SHADE_MIN of them can be shaded together.  Between
// bounces a lane keeps its item, its step, the running colour and the specular bit; origin and direction live in the
// traversal state.  A ghost re-reads the record it copies from the lane's own previous plane (step 0: from `first`), so
// the 24-word payload is not held across the traversal.
#include "kernels.h"

#include "device_item_loop.hpp"
#include "device_math.hpp"
#include "device_query.hpp"
#include "device_scene.hpp"
#include "launch.hpp"

namespace bdpt {

namespace {

// step `s` of item `i` does not exist, or its `samples` / `hits` are a ghost's: zeros, prim -1
__device__ __forceinline__ void walkWriteNoSample(const WalkQueryDev& Q, size_t at) {
  const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (Q.samples) {
    Q.samples[at * 2] = z;
    Q.samples[at * 2 + 1] = z;
  }
  if (Q.hits) Q.hits[at] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
}
__device__ __forceinline__ void walkWriteNone(const WalkQueryDev& Q, uint32_t from, uint32_t i) {
  const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (uint32_t s = from; s < Q.steps; s++) {
    const size_t at = (size_t)s * Q.range.cap + i;
    float4* o = Q.vertices + at * 6;
    o[0] = z;
    o[1] = z;
    o[2] = z;
    o[3] = z;
    o[4] = z;
    o[5] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
    Q.info[at] = z;
    walkWriteNoSample(Q, at);
  }
}

}  // namespace

// Waves per SIMD the register allocation aims for (experiment knob, as BDPT_WALK_WAVES_PER_EU of walk_kernel): 4 is what the
// kernel needs without spilling (DESIGN.md "Walk queries" has the register counts of 5 and 6).
#ifndef BDPT_WALKQ_WAVES_PER_EU
#define BDPT_WALKQ_WAVES_PER_EU 4
#endif
// Lanes whose ray is answered wait ("parked": they keep their slot but take no traversal step) until this many of the wave
// wait, or no lane is traversing: hit shading and sampling are some thousand instructions, and after every leaf phase
// (BDPT_WALKQ_SHADE_MIN 1) they ran for the handful of lanes that phase finished.  Measured with tools/walk_query_times.py
// (DESIGN.md "Walk queries"): 1, 8, 16, 24, 32 waiting lanes give 5.96, 5.61, 5.01, 4.77, 4.68 ms.
#ifndef BDPT_WALKQ_SHADE_MIN
#define BDPT_WALKQ_SHADE_MIN 32
#endif
// starts[3i] = (org, tmin), starts[3i+1] = (dir, tmax), starts[3i+2] = (colour, unused) (bdpt_walk_start); plane s of item i
// at s * cap + i: vertices six float4 (bdpt_surface), info (colour, status), samples two float4, hits one.
// cursor: as releaseCursor has it (both words zero when a launch starts and when it ends).
template <bool GGX>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(BDPT_WALKQ_WAVES_PER_EU, 8))) void walk_query_kernel(
    SceneDev S, WalkQueryDev Q, bool fromLobe, unsigned long long* cursor) {
  BDPT_ONE_WAVE_PER_GROUP();
  __shared__ int s_stack[kStackLds * kWave];
  int* stk = s_stack + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const uint32_t cap = Q.range.cap;
  ItemFeed F = feedInit(itemCount(cap, Q.range.count));
  bool has = false, parked = false;
  uint32_t rid = 0, step = 0;
  f3 pcolor = mk(0);
  bool pspec = false;
  TravState T;
  T.cur = kDone;
  while (refill(F, cursor, lane, has, [&](uint32_t item) {
    rid = item;
    if (Q.alive && Q.alive[rid] == 0) {
      walkWriteNone(Q, 0u, rid);  // no path: the lane stays idle
    } else {
      const float4 a = Q.starts[(size_t)rid * 3], b = Q.starts[(size_t)rid * 3 + 1], c = Q.starts[(size_t)rid * 3 + 2];
      float4 org = a;
      if (Q.first) org = Q.first[(size_t)rid * 6];
      pcolor = mk(c.x, c.y, c.z);
      pspec = Q.firstSpecular ? Q.firstSpecular[rid] != 0 : false;
      step = 0;
      travInit(T, mk(org.x, org.y, org.z), mk(b.x, b.y, b.z), a.w, b.w);
      has = true;
    }
  })) {
    const bool leavesDue = nodePhase<1>(S, T, stk, has && !parked);
    if (leavesDue && has && !parked && T.cur < 0) parked = leafPhase<BDPT_TRACE_CLOSEST>(S, T, stk);
    // the parked lanes, together (parkedDue): vertex `step` of their item
    if (parkedDue<BDPT_WALKQ_SHADE_MIN>(parked, has && !parked) && parked) {
      parked = false;
      const size_t at = (size_t)step * cap + rid;
      float4* o = Q.vertices + at * 6;
      const int prim = T.best.prim;
      if (prim >= 0) {
        const f3 ro = T.o;
        const Shading sd = shadeHit<false>(S, (uint32_t)prim, T.best.u, T.best.v, ro);
        const uint32_t matId = __float_as_uint(S.shade[(size_t)prim * kShadeRecF4 + 6].x);
        // the record as shade_hits_kernel writes it, and the sample as bsdf_query_kernel draws it from those words
        const float4 q0 = make_float4(sd.posW.x, sd.posW.y, sd.posW.z, length(sd.posW - ro));
        const float4 q1 = make_float4(sd.N.x, sd.N.y, sd.N.z, sd.linearRoughness);
        const float4 q2 = make_float4(sd.V.x, sd.V.y, sd.V.z, sd.IoR);
        const float4 q3 = make_float4(sd.diffuse.x, sd.diffuse.y, sd.diffuse.z, sd.opacity);
        const float4 q4 = make_float4(sd.specular.x, sd.specular.y, sd.specular.z, __uint_as_float(matId));
        const float4 q5 = make_float4(sd.emissive.x, sd.emissive.y, sd.emissive.z, __int_as_float(prim));
        const uint32_t seed = Q.seeds[Q.seedPerStep ? at : (size_t)rid];
        const f3 N = mk(q1.x, q1.y, q1.z), V = mk(q2.x, q2.y, q2.z), D = mk(q3.x, q3.y, q3.z), Sp = mk(q4.x, q4.y, q4.z);
        const float rough = q1.w * q1.w;
        f3 L = mk(0);
        float pdf = 0.0f;
        bool isSpec = false;
        const f3 w = sampleBRDF<GGX>(seed, N, N, V, D, Sp, rough, fromLobe, L, pdf, isSpec);
        pcolor = pcolor * w;
        pspec = isSpec;
        o[0] = q0;
        o[1] = q1;
        o[2] = q2;
        o[3] = q3;
        o[4] = q4;
        o[5] = q5;
        Q.info[at] = make_float4(pcolor.x, pcolor.y, pcolor.z,
                                 __uint_as_float(BDPT_WALK_STATUS_STORED | BDPT_WALK_STATUS_REAL | (isSpec ? BDPT_WALK_STATUS_SPECULAR : 0u)));
        if (Q.samples) {
          Q.samples[at * 2] = make_float4(L.x, L.y, L.z, pdf);
          Q.samples[at * 2 + 1] = make_float4(w.x, w.y, w.z, __uint_as_float(isSpec ? 1u : 0u));
        }
        if (Q.hits) Q.hits[at] = make_float4(T.best.t, T.best.u, T.best.v, __int_as_float(prim));
        step++;
        if (step < Q.steps) {
          travInit(T, mk(q0.x, q0.y, q0.z), L, Q.range.minT, 1e+38f);  // the lane keeps its slot
        } else {
          has = false;
          T.cur = kDone;
        }
      } else {
        // a ghost: a copy of its predecessor (the lane's own previous vertex; step 0: `first`, or only the origin)
        const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float4 g0 = make_float4(T.o.x, T.o.y, T.o.z, 0.0f), g1 = z, g2 = z, g3 = z, g4 = z, g5 = z;
        const float4* src = step ? Q.vertices + ((size_t)(step - 1) * cap + rid) * 6 : (Q.first ? Q.first + (size_t)rid * 6 : nullptr);
        if (src) {
          g0 = src[0];
          g1 = src[1];
          g2 = src[2];
          g3 = src[3];
          g4 = src[4];
          g5 = src[5];
        }
        const int gp = __float_as_int(g5.w);
        g5.w = __int_as_float(gp > 0 ? gp : 0);
        o[0] = g0;
        o[1] = g1;
        o[2] = g2;
        o[3] = g3;
        o[4] = g4;
        o[5] = g5;
        Q.info[at] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(BDPT_WALK_STATUS_STORED | (pspec ? BDPT_WALK_STATUS_SPECULAR : 0u)));
        walkWriteNoSample(Q, at);
        walkWriteNone(Q, step + 1u, rid);
        has = false;
        T.cur = kDone;
      }
    }
  }
  releaseCursor(cursor, lane);
}

void launchWalkQuery(const SceneDev& S, const WalkQueryDev& Q, bool ggx, bool fromLobe, unsigned long long* cursor, LaunchGrids& G,
                     int numCUs, hipStream_t st) {
  if (!Q.range.cap) return;
  withFlag(ggx, [&](auto GGX) {
    launchPersistent(walk_query_kernel<GGX>, G.walkQuery[GGX ? 1 : 0], Q.range.cap, numCUs, st, S, Q, fromLobe, cursor);
  });
}

}  // namespace bdpt
