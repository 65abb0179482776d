// device_area.hpp — sampling the emitter table of BDPT_PARAM_AREA_LIGHTS (contract: include/bdpt.h "Area lights").
// The AREA instances of init_paths and gen_nee and the test hook bdpt_test_area_light_sample call these functions, so
// the hook sees exactly what a frame computes.
#pragma once
#include "device_math.hpp"
#include "device_scene.hpp"
#include "kernels.h"

namespace bdpt {
#define BD __device__ __forceinline__

constexpr uint32_t kAreaStreamKey = 0x41524541u;  // "AREA": initRand(state, key) seeds a NEE term's three area uniforms

// W of the table (the refresh writes it beside the fallback emitter)
BD float areaTotal(const AreaDev& A) { return A.total[0]; }

// Emitter i: the first whose CDF value is greater than a * W (binary search); none (rounding at the top): the last
// emitter with a positive weight
BD uint32_t areaPick(const AreaDev& A, float W, float a) {
  const float target = a * W;
  uint32_t lo = 0, hi = A.n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (A.cdf[mid] > target)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo < A.n ? lo : __float_as_uint(A.total[1]);
}

struct AreaPoint {
  uint32_t prim;
  float b1, b2;
  f3 pos, ng, Le;
  float pA;  // area pdf w_i / (W * area_i)
};
// The point of uniforms (a, u1, u2): barycentrics b1 = u2 sqrt(u1), b2 = 1 - sqrt(u1); position and emission as shadeHit
// gives them there (the same texture fetch); emission zero where the alpha test fails or the geometric normal has zero
// length.
BD AreaPoint areaPoint(const SceneDev& S, const AreaDev& A, float W, float a, float u1, float u2) {
  const uint32_t i = areaPick(A, W, a);
  const float4 e = A.emit[i];
  AreaPoint r;
  r.prim = __float_as_uint(e.x);
  const uint32_t alphaRec = __float_as_uint(e.y);
  const float su = sqrtf(u1);
  r.b1 = u2 * su;
  r.b2 = 1.0f - su;
  const Shading sd = shadeHit<false>(S, r.prim, r.b1, r.b2, mk(0));
  r.pos = sd.posW;
  r.Le = sd.emissive;
  const float4* sr = S.shade + (size_t)r.prim * kShadeRecF4;
  const float4 q0 = sr[0], q2 = sr[2], q4 = sr[4];
  const f3 p0 = mk(q0.x, q0.y, q0.z), p1 = mk(q2.x, q2.y, q2.z), p2 = mk(q4.x, q4.y, q4.z);
  const f3 c = cross(p1 - p0, p2 - p0);
  const bool flat = !(dot(c, c) > 0.0f);
  r.ng = flat ? mk(0) : normalize(c);
  if (flat || (alphaRec != kNoAlphaRec && alphaTestFails(S, alphaRec, r.b1, r.b2))) r.Le = mk(0);
  r.pA = e.z / (W * e.w);
  return r;
}

BD bool finite3(f3 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }

// Light subpath start (init_paths, after the selection draw): draws a, u1, u2, the side s and the cosine direction from
// `seed`.  colour = Le * 2 pi / p_A (two-sided cosine emission: Le |cos| / (p_A p_omega)); +0 where that is not finite.
BD AreaPoint areaLightStart(const SceneDev& S, const AreaDev& A, float W, uint32_t& seed, f3& n, f3& dir, f3& color) {
  const float a = nextRand(seed);
  const float u1 = nextRand(seed);
  const float u2 = nextRand(seed);
  const float s = nextRand(seed);
  const AreaPoint x = areaPoint(S, A, W, a, u1, u2);
  n = s < 0.5f ? x.ng : -x.ng;
  dir = getCosHemisphereSample(seed, n);
  color = x.Le * ((2.0f * kPi) / x.pA);
  if (!finite3(color)) color = mk(0);
  return x;
}

// NEE sample towards the table for a receiving point `pos`; `state` is the seed after the term's selection draw.
// L = (x - pos) / d; intensity = Le |dot(n_g, L)| / (p_A d^2), +0 when d^2 == 0 or the value is not finite.
BD AreaPoint areaNee(const SceneDev& S, const AreaDev& A, float W, uint32_t state, f3 pos, f3& L, float& d, f3& intensity) {
  uint32_t sa = initRand(state, kAreaStreamKey);
  const float a = nextRand(sa);
  const float u1 = nextRand(sa);
  const float u2 = nextRand(sa);
  const AreaPoint x = areaPoint(S, A, W, a, u1, u2);
  const f3 v = x.pos - pos;
  const float d2 = dot(v, v);
  d = sqrtf(d2);
  L = d2 > 0.0f ? v / d : mk(0);
  intensity = x.Le * (fabsf(dot(x.ng, L)) / (x.pA * d2));
  if (!(d2 > 0.0f) || !finite3(intensity)) intensity = mk(0);
  return x;
}

#undef BD
}  // namespace bdpt
