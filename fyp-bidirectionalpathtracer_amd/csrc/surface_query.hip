// surface_query.hip — bdpt_camera_rays, bdpt_shade_hits and bdpt_bsdf_query: the G-buffer pass's primary rays, the pass's
// hit shading and its BSDF, on a caller's arrays in device memory.
//
// With them a caller's own integrator runs camera rays -> bdpt_trace_rays -> shade -> sample -> trace on the device with
// the pass's arithmetic: every kernel here calls the device function the pass itself calls (primaryRay, shadeHit,
// sampleBRDF, evalBRDF), none restates it.  There is no traversal, so no persistent grid: one lane per item on a dense
// grid of one-wave workgroups; a lane past the item count returns.
#include "kernels.h"

#include "device_math.hpp"
#include "device_query.hpp"
#include "device_scene.hpp"
#include "device_trace.hpp"  // BDPT_ONE_WAVE_PER_GROUP
#include "launch.hpp"

namespace bdpt {

// rays[2i] = (org, 0), rays[2i+1] = (dir, 1e38) for pixel i = x + y * W (bdpt_ray)
__global__ __launch_bounds__(kWave) void camera_rays_kernel(bdpt_camera cam, bdpt_gbuffer_params gp, uint32_t W, uint32_t H,
                                                            float4* __restrict__ rays) {
  BDPT_ONE_WAVE_PER_GROUP();
  const uint32_t i = blockIdx.x * kWave + threadIdx.x;
  if (i >= W * H) return;
  const uint32_t y = i / W, x = i - y * W;
  f3 o, d;
  primaryRay(cam, gp, x, y, W, H, o, d);
  rays[(size_t)i * 2] = make_float4(o.x, o.y, o.z, 0.0f);
  rays[(size_t)i * 2 + 1] = make_float4(d.x, d.y, d.z, 1e+38f);
}

// bdpt_surface: six float4 per hit, (posW, dist) (N, linearRoughness) (V, IoR) (diffuse, opacity) (specular, material)
// (emissive, prim).  A miss, or a prim outside the scene, writes prim -1, material 0xffffffff and zeros.
template <bool NMAP>
__global__ __launch_bounds__(kWave) void shade_hits_kernel(SceneDev S, uint32_t numTris, const float4* __restrict__ rays,
                                                           const float4* __restrict__ hits, uint32_t cap, const uint32_t* count,
                                                           float4* __restrict__ out) {
  BDPT_ONE_WAVE_PER_GROUP();
  uint32_t i;
  if (queryLanePast(cap, count, i)) return;
  const float4 org = rays[(size_t)i * 2], h = hits[i];
  const int prim = __float_as_int(h.w);
  float4* o = out + (size_t)i * 6;
  if (prim < 0 || (uint32_t)prim >= numTris) {
    const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    o[0] = z;
    o[1] = z;
    o[2] = z;
    o[3] = z;
    o[4] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xffffffffu));
    o[5] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
    return;
  }
  const f3 ro = mk(org.x, org.y, org.z);
  const Shading sd = shadeHit<NMAP>(S, (uint32_t)prim, h.y, h.z, ro);  // the ray origin as camPosW, as the walk passes it
  const uint32_t matId = __float_as_uint(S.shade[(size_t)prim * kShadeRecF4 + 6].x);
  o[0] = make_float4(sd.posW.x, sd.posW.y, sd.posW.z, length(sd.posW - ro));
  o[1] = make_float4(sd.N.x, sd.N.y, sd.N.z, sd.linearRoughness);
  o[2] = make_float4(sd.V.x, sd.V.y, sd.V.z, sd.IoR);
  o[3] = make_float4(sd.diffuse.x, sd.diffuse.y, sd.diffuse.z, sd.opacity);
  o[4] = make_float4(sd.specular.x, sd.specular.y, sd.specular.z, __uint_as_float(matId));
  o[5] = make_float4(sd.emissive.x, sd.emissive.y, sd.emissive.z, __int_as_float(prim));
}

// SAMPLE (EVAL = false): sampleBRDF with the item's seed -> samples[2i] = (L, pdf), samples[2i+1] = (weight, isSpecular);
// EVAL: evalBRDF towards dirs[i].xyz (dirs[i].w != 0: the sampled lobe was specular) -> values[i] = (f, 0).
// Reads the record's N, V, diffuse, specular, linearRoughness and prim only.
template <bool GGX, bool EVAL>
__global__ __launch_bounds__(kWave) void bsdf_query_kernel(const float4* __restrict__ surf, uint32_t cap, const uint32_t* count,
                                                           bool fromLobe, const uint32_t* __restrict__ seeds,
                                                           const float4* __restrict__ dirs, float4* __restrict__ out) {
  BDPT_ONE_WAVE_PER_GROUP();
  uint32_t i;
  if (queryLanePast(cap, count, i)) return;
  const float4* r = surf + (size_t)i * 6;
  const int prim = __float_as_int(r[5].w);
  const float4 n = r[1], v = r[2], dif = r[3], spec = r[4];
  const f3 N = mk(n.x, n.y, n.z), V = mk(v.x, v.y, v.z), D = mk(dif.x, dif.y, dif.z), Sp = mk(spec.x, spec.y, spec.z);
  const float rough = n.w * n.w;  // shadeHit's roughness from linearRoughness
  if (EVAL) {
    const float4 l = dirs[i];
    f3 f = mk(0);
    if (prim >= 0) f = evalBRDF<GGX>(V, mk(l.x, l.y, l.z), N, N, D, Sp, rough, l.w != 0.0f);
    out[i] = make_float4(f.x, f.y, f.z, 0.0f);
  } else {
    f3 L = mk(0), w = mk(0);
    float pdf = 0.0f;
    bool isSpec = false;
    if (prim >= 0) w = sampleBRDF<GGX>(seeds[i], N, N, V, D, Sp, rough, fromLobe, L, pdf, isSpec);
    out[(size_t)i * 2] = make_float4(L.x, L.y, L.z, pdf);
    out[(size_t)i * 2 + 1] = make_float4(w.x, w.y, w.z, __uint_as_float(isSpec ? 1u : 0u));
  }
}

void launchCameraRays(const bdpt_camera& cam, const bdpt_gbuffer_params& gp, uint32_t W, uint32_t H, float4* rays, hipStream_t st) {
  const uint32_t n = W * H;
  if (!n) return;
  launchWave(camera_rays_kernel, wavesFor(n), st, cam, gp, W, H, rays);
}

void launchShadeHits(const SceneDev& S, uint32_t numTris, const float4* rays, const float4* hits, uint32_t cap, const uint32_t* count,
                     bool normalMap, float4* out, hipStream_t st) {
  if (!cap) return;
  withFlag(normalMap, [&](auto NMAP) { launchWave(shade_hits_kernel<NMAP>, wavesFor(cap), st, S, numTris, rays, hits, cap, count, out); });
}

void launchBsdfQuery(const float4* surf, uint32_t cap, const uint32_t* count, bool eval, bool ggx, bool fromLobe, const uint32_t* seeds,
                     const float4* dirs, float4* out, hipStream_t st) {
  if (!cap) return;
  withFlag(ggx, [&](auto GGX) {
    withFlag(eval, [&](auto EVAL) {
      launchWave(bsdf_query_kernel<GGX, EVAL>, wavesFor(cap), st, surf, cap, count, fromLobe, seeds, dirs, out);
    });
  });
}

}  // namespace bdpt
