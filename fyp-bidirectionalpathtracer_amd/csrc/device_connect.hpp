// device_connect.hpp — the arithmetic of the two strategies that join a light vertex to the eye side: a vertex
// connection (BDPTMain.rt.hlsl:212-233, evalGWithoutV / getUnweightedContribution BDPTUtils.hlsli:172-224) and a
// light-tracing splat (BDPTMain.rt.hlsl:171-208, getLaunchIndexFromDirection BDPTUtils.hlsli:129-138).
// gen_connect_kernel, gen_splat_kernel and lazy_gen_kernel of kernels.hip and the query kernels of connect_query.hip call
// these; none restates them.  A vertex is anything with pos, N, dif, spec, rough and isSpec (kernels.hip's Vtx, or the
// fields of a bdpt_surface record).
#pragma once
#include "device_math.hpp"

namespace bdpt {
#define BD __device__ __forceinline__

// The ray of a pair, eye vertex -> light vertex, as gen_connect and the lazy rounds form it: coincident points give
// tmax 0 and a NaN direction, which the traversal answers "miss".
BD void pairRay(f3 eyePos, f3 lightPos, f3& dirAB, float& lengthAB) {
  lengthAB = length(lightPos - eyePos);
  dirAB = (lightPos - eyePos) / lengthAB;
}

// (fsL * G) * fsE of a pair.  woE / woL: the directions from the two vertices to their predecessors.  Returns false where
// a short cut was taken (fsL all zero: value = fsL; else fsE all zero: value = fsE): the pass then skips the path colours.
template <bool GGX, class V>
BD bool pairValue(const V& ev, f3 woE, const V& le, f3 woL, f3& value) {
  const f3 vecAB = le.pos - ev.pos;
  const float invLengthAB = 1.0f / length(vecAB);
  const f3 dirG = vecAB * invLengthAB;
  const float cosA = fabsf(dot(ev.N, dirG));
  const float cosB = fabsf(dot(le.N, dirG));
  const float Gt = cosA * cosB * invLengthAB * invLengthAB;
  const f3 connectDir = normalize(ev.pos - le.pos);
  const f3 fsL = evalBRDF<GGX>(connectDir, woL, le.N, le.N, le.dif, le.spec, le.rough, le.isSpec);
  if (allZero(fsL)) {
    value = fsL;
    return false;
  }
  const f3 fsE = evalBRDF<GGX>(-connectDir, woE, ev.N, ev.N, ev.dif, ev.spec, ev.rough, ev.isSpec);
  if (allZero(fsE)) {
    value = fsE;
    return false;
  }
  value = (fsL * Gt) * fsE;
  return true;
}

// The camera as the splat sees it (wave-uniform).
struct SplatCam {
  f3 pos, U, V, W, N;  // N = normalize(W)
};
BD SplatCam splatCam(const bdpt_camera& cam) {
  SplatCam c;
  c.pos = ld3(cam.posW);
  c.U = ld3(cam.cameraU);
  c.V = ld3(cam.cameraV);
  c.W = ld3(cam.cameraW);
  c.N = normalize(c.W);
  return c;
}

// The pixel a direction towards the camera lands in: true when the vertex faces the camera and the target lies inside the
// W x H frame (fx, fy are then its integer coordinates).  jx, jy: the frame's pixel jitter.
BD bool splatTarget(const SplatCam& c, f3 dirToCamera, uint32_t W, uint32_t H, float jx, float jy, float& fx, float& fy) {
  if (!(dot(c.N, dirToCamera) < 0)) return false;
  float d1 = dot(dirToCamera, c.U) / dot(c.U, c.U);
  float d2 = dot(dirToCamera, c.V) / dot(c.V, c.V);
  float d3 = dot(dirToCamera, c.W) / dot(c.W, c.W);
  float nx = d1 / d3, ny = -d2 / d3;
  float px = nx * 0.5f + 0.5f, py = ny * 0.5f + 0.5f;
  fx = rintf(px * (float)W - jx);
  fy = rintf(py * (float)H - jy);
  return fx >= 0.0f && fx < (float)W && fy >= 0.0f && fy < (float)H;
}

// The two factors of a splat: fr = evalBRDF(V, dirToCamera, ...) and the geometry term.  The pass forms
// (prevColor * fr) * Gt, which is not prevColor * (fr * Gt) in fp32, so they stay apart.
template <bool GGX, class Vx>
BD void splatTerm(const SplatCam& c, const Vx& lv, f3 vV, f3 dirToCamera, float disToCamera, f3& fr, float& Gt) {
  float theta1 = saturate(fabsf(dot(dirToCamera, c.N)));
  float theta2 = saturate(fabsf(dot(dirToCamera, lv.N)));
  float invDisToCamera = 1.0f / disToCamera;
  Gt = theta1 * theta2 * invDisToCamera * invDisToCamera;
  fr = evalBRDF<GGX>(vV, dirToCamera, lv.N, lv.N, lv.dif, lv.spec, lv.rough, lv.isSpec);
}

#undef BD
}  // namespace bdpt
