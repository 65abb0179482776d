// device_light.hpp — one next-event candidate of the pass on a caller's surface point: the text bdpt_light_query(NEE)
// (light_query.hip), the resampled direct lighting kernel (ris.hip) and its reuse stage (reuse.hip) share.  It is the light part of genNeeLane
// (kernels.hip, which keeps its own text): the uniform light choice from one draw, getLightData or the emitter table's
// areaNee, and directIfVisible.  Every step is the pass's own device function; nothing is restated here.
#pragma once
#include "device_area.hpp"
#include "device_math.hpp"
#include "device_scene.hpp"

namespace bdpt {
#define BD __device__ __forceinline__

// the light count of the pass: the emitter table is light numLights of numLights + 1 while its W is positive
template <bool AREA>
BD int lightsCountOf(const SceneDev& S, const AreaDev& A, float& areaW) {
  areaW = AREA ? areaTotal(A) : 0.0f;
  return (int)S.numLights + ((AREA && areaW > 0.0f) ? 1 : 0);
}

// What a candidate is, beside its value: the light, whether that is the emitter table, and the shadow ray's direction and
// length (the ray starts at the surface point with the caller's tmin).
struct LightCandidate {
  int light;
  bool area;
  f3 L;
  float dist;
};

// The candidate that is light `lightToSample` (0 .. lightsCount - 1: the caller checks) at `pos`; `state` is the RNG state
// after the selection draw that chose it, from which areaNee forks its three uniforms (by value: the caller's state does
// not advance).  The emitter point does not depend on `pos`, so (light, state) names one light sample for every receiver:
// what reservoir reuse (reuse.hip) re-evaluates.  Returns the unweighted, unclamped value of a visible light,
// bdpt_light_sample::value.  V, spec and rough are read by the GGX form only.
template <bool GGX, bool AREA>
BD f3 lightGiven(const SceneDev& S, const AreaDev& A, float areaW, int lightsCount, int lightToSample, uint32_t state, f3 pos, f3 N, f3 V,
                 f3 dif, f3 spec, float rough, LightCandidate& c) {
  f3 L, lightIntensity;
  float distToLight;
  const bool area = AREA && lightToSample == (int)S.numLights;
  if (area) {
    areaNee(S, A, areaW, state, pos, L, distToLight, lightIntensity);
    distToLight = distToLight * (1.0f - 1e-4f);  // the emitter does not occlude its own sample
  } else {
    getLightData(S.sc->lights[lightToSample], pos, L, lightIntensity, distToLight);
  }
  c.light = lightToSample;
  c.area = area;
  c.L = L;
  c.dist = distToLight;
  return directIfVisible<GGX>((float)lightsCount, L, lightIntensity, N, V, dif, spec, rough);
}

// The candidate of selection draw `r` at `pos`: the uniform light choice, then lightGiven (`state`: after that draw).
template <bool GGX, bool AREA>
BD f3 lightCandidate(const SceneDev& S, const AreaDev& A, float areaW, int lightsCount, float r, uint32_t state, f3 pos, f3 N, f3 V,
                     f3 dif, f3 spec, float rough, LightCandidate& c) {
  int lightToSample = (int)(r * (float)lightsCount);
  if (lightToSample > lightsCount - 1) lightToSample = lightsCount - 1;
  return lightGiven<GGX, AREA>(S, A, areaW, lightsCount, lightToSample, state, pos, N, V, dif, spec, rough, c);
}

#undef BD
}  // namespace bdpt
