// light_query.hip — bdpt_light_query: the pass's light sampling on a caller's arrays in device memory.
//
//   BDPT_LIGHT_NEE   the light part of genNeeLane (kernels.hip): the uniform light choice, getLightData or the emitter
//                    table's areaNee, directIfVisible, and the occluder hint of a point / spot light
//   BDPT_LIGHT_EMIT  sampleLight of initPathsLane: the start of a light subpath
//
// With the surface queries and bdpt_trace_rays a forward path tracer with next-event estimation is a sequence of calls on
// one stream.  Every kernel here calls the device function the pass itself calls (getLightData, areaNee, areaLightStart,
// directIfVisible, recOccludes, lightHint, sampleUnitSphere, getCosHemisphereSample), none restates it.  There is no
// traversal, so no persistent grid: one lane per item on a dense grid of one-wave workgroups.  A lane past the item count
// returns, except in the COMPACT instances, where it stays for the wave's ballot (a wave wholly past the count returns).
#include "kernels.h"

#include "device_area.hpp"
#include "device_light.hpp"
#include "device_math.hpp"
#include "device_query.hpp"
#include "device_scene.hpp"
#include "device_trace.hpp"  // BDPT_ONE_WAVE_PER_GROUP, recOccludes, lightHint
#include "launch.hpp"

namespace bdpt {

namespace {
// bdpt_light_sample: three float4 per item, (org, tmin) (dir, tmax) (value, light | status << 16).  Reads the record's
// posW, N, linearRoughness, diffuse and prim, and for GGX also V and specular (the Lambertian value uses neither, as
// gen_nee's loadSurf<false> leaves them zero).
template <bool GGX, bool AREA, bool HINTS, bool COMPACT>
__device__ __forceinline__ void lightNeeLane(const SceneDev& S, const LightQueryDev& Q, const AreaDev& A) {
  uint32_t i, n;
  if (queryLanePast<COMPACT>(Q.range.cap, Q.range.count, i, n)) return;
  const bool act = i < n;
  bool emit = false;
  float4 q0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), q1 = q0;
  if (act) {
    float areaW;
    const int lightsCount = lightsCountOf<AREA>(S, A, areaW);
    uint32_t seed = Q.seeds[i];
    const float r = nextRand(seed);  // the term's one draw, also for a record that is a miss
    if (Q.seedsOut) Q.seedsOut[i] = seed;
    const float4* rec = Q.surf + (size_t)i * 6;
    float4 q2 = q0;
    if (__float_as_int(rec[5].w) >= 0) {
      const float4 p = rec[0], nr = rec[1], dif = rec[3];
      const f3 pos = mk(p.x, p.y, p.z);
      f3 V = mk(0), spec = mk(0);
      float rough = 0.0f;
      if (GGX) {
        const float4 v = rec[2], sp = rec[4];
        V = mk(v.x, v.y, v.z);
        spec = mk(sp.x, sp.y, sp.z);
        rough = nr.w * nr.w;  // shadeHit's roughness from linearRoughness
      }
      LightCandidate cand;
      const f3 value = lightCandidate<GGX, AREA>(S, A, areaW, lightsCount, r, seed, pos, mk(nr.x, nr.y, nr.z), V, mk(dif.x, dif.y, dif.z),
                                                 spec, rough, cand);
      const int lightToSample = cand.light;
      const bool area = cand.area;
      const f3 L = cand.L;
      const float distToLight = cand.dist;
      uint32_t status = allZero(value) ? 0u : BDPT_LIGHT_STATUS_NONZERO;
      // The nearest triangle the light sees towards this point is tried first, exactly as gen_nee tries it.  gen_nee tests
      // its clamped term, which is zero for a value without a positive component (NaN where NdotV is 0, or a negative
      // intensity) whatever the throughput and weight: such a value is not ±0, so it keeps bit 0, but no hint is tried.
      const bool positive = value.x > 0.0f || value.y > 0.0f || value.z > 0.0f;
      if (HINTS && positive && !area && S.sc->lights[lightToSample].type != BDPT_LIGHT_DIRECTIONAL &&
          recOccludes(S, lightHint(S, lightToSample, ld3(S.sc->lights[lightToSample].posW), pos), pos, L, Q.range.minT, distToLight))
        status |= BDPT_LIGHT_STATUS_HINT_OCCLUDED;
      emit = status == BDPT_LIGHT_STATUS_NONZERO;
      q0 = make_float4(pos.x, pos.y, pos.z, Q.range.minT);
      q1 = make_float4(L.x, L.y, L.z, distToLight);
      q2 = make_float4(value.x, value.y, value.z, __uint_as_float((uint32_t)lightToSample | (status << 16)));
    }
    float4* o = Q.out + (size_t)i * 3;
    o[0] = q0;
    o[1] = q1;
    o[2] = q2;
  }
  if (COMPACT) compactAppend(Q.compact, Q.range.cap, emit, i, q0, q1);
}

// bdpt_light_emit: three float4 per item, (org, tmin) (dir, 1e38) (colour, light); seedsOut = the pass's seedL
template <bool AREA>
__device__ __forceinline__ void lightEmitLane(const SceneDev& S, const LightQueryDev& Q, const AreaDev& A) {
  uint32_t i;
  if (queryLanePast(Q.range.cap, Q.range.count, i)) return;
  float areaW;
  const int lightsCount = lightsCountOf<AREA>(S, A, areaW);
  uint32_t seed = Q.seeds[i];
  int index = (int)(nextRand(seed) * (float)lightsCount);
  if (index > lightsCount - 1) index = lightsCount - 1;
  f3 lightDir, pos, color;
  if (AREA && index == (int)S.numLights) {
    f3 nrm;
    pos = areaLightStart(S, A, areaW, seed, nrm, lightDir, color).pos;
  } else {
    const bdpt_light& l = S.sc->lights[index];
    if (l.type == BDPT_LIGHT_DIRECTIONAL)
      lightDir = ld3(l.dirW);
    else
      lightDir = sampleUnitSphere(seed);
    lightDir = getCosHemisphereSample(seed, lightDir);
    pos = ld3(l.posW);
    color = ld3(l.intensity);
  }
  if (Q.seedsOut) Q.seedsOut[i] = seed;
  float4* o = Q.out + (size_t)i * 3;
  o[0] = make_float4(pos.x, pos.y, pos.z, Q.range.minT);
  o[1] = make_float4(lightDir.x, lightDir.y, lightDir.z, 1e+38f);
  o[2] = make_float4(color.x, color.y, color.z, __uint_as_float((uint32_t)index));
}
}  // namespace

template <bool GGX, bool HINTS, bool COMPACT>
__global__ __launch_bounds__(kWave) void light_nee_kernel(SceneDev S, LightQueryDev Q) {
  BDPT_ONE_WAVE_PER_GROUP();
  lightNeeLane<GGX, false, HINTS, COMPACT>(S, Q, AreaDev{});
}
// the AREA instances: the emitter table as one more argument, as gen_nee_area_kernel takes it
template <bool GGX, bool HINTS, bool COMPACT>
__global__ __launch_bounds__(kWave) void light_nee_area_kernel(SceneDev S, LightQueryDev Q, AreaDev A) {
  BDPT_ONE_WAVE_PER_GROUP();
  lightNeeLane<GGX, true, HINTS, COMPACT>(S, Q, A);
}
__global__ __launch_bounds__(kWave) void light_emit_kernel(SceneDev S, LightQueryDev Q) {
  BDPT_ONE_WAVE_PER_GROUP();
  lightEmitLane<false>(S, Q, AreaDev{});
}
__global__ __launch_bounds__(kWave) void light_emit_area_kernel(SceneDev S, LightQueryDev Q, AreaDev A) {
  BDPT_ONE_WAVE_PER_GROUP();
  lightEmitLane<true>(S, Q, A);
}

void launchLightQuery(const SceneDev& S, const LightQueryDev& Q, const AreaDev& A, bool emitMode, bool ggx, bool hints, hipStream_t st) {
  if (!Q.range.cap) return;
  const uint32_t g = wavesFor(Q.range.cap);
  if (emitMode) {
    if (A.n)
      launchWave(light_emit_area_kernel, g, st, S, Q, A);
    else
      launchWave(light_emit_kernel, g, st, S, Q);
    return;
  }
  withFlag(ggx, [&](auto GGX) {
    withFlag(hints, [&](auto HINTS) {
      withFlag(Q.compact.rays != nullptr, [&](auto COMPACT) {
        if (A.n)
          launchWave(light_nee_area_kernel<GGX, HINTS, COMPACT>, g, st, S, Q, A);
        else
          launchWave(light_nee_kernel<GGX, HINTS, COMPACT>, g, st, S, Q);
      });
    });
  });
}

}  // namespace bdpt
