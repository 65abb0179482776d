// connect_query.hip — bdpt_connect_query and bdpt_splat_add: the pass's vertex connections and light tracing on a
// caller's arrays in device memory.
//
//   BDPT_CONNECT_VERTICES  the pair arithmetic of gen_connect_kernel (kernels.hip): the ray lazy_gen_kernel shares with it
//                          and (fsL * G) * fsE with the kernel's short cuts
//   BDPT_CONNECT_CAMERA    gen_splat_kernel without the path buffers: the ray to the camera, f, G and the target pixel
//   bdpt_splat_add         the splat half of gatherLane: fixed-point atomics into a uint64[4]-per-pixel buffer
//
// With the other queries every strategy of the pass is a sequence of calls on one stream.  The kernels call the device
// functions the pass calls (device_connect.hpp: pairRay, pairValue, splatTarget, splatTerm; toFixed), none restates them.
// No traversal, so no persistent grid: one lane per item on a dense grid of one-wave workgroups.  A lane past the item
// count returns, except in the COMPACT instances, where it stays for the wave's ballot (a wave wholly past it returns).
#include "kernels.h"

#include "device_connect.hpp"
#include "device_math.hpp"
#include "device_query.hpp"
#include "device_trace.hpp"  // BDPT_ONE_WAVE_PER_GROUP
#include "launch.hpp"

namespace bdpt {

namespace {
// the fields of a bdpt_surface record the BSDF reads (the names pairValue / splatTerm expect)
struct SurfVtx {
  f3 pos, N, dif, spec;
  float rough;
  bool isSpec;
};
// rec: six float4.  Lambertian evalBRDF returns dif: specular, roughness and the flag stay zero and are never loaded.
template <bool GGX>
__device__ __forceinline__ SurfVtx loadSurfVtx(const float4* rec, const uint8_t* specular, uint32_t i) {
  const float4 p = rec[0], nr = rec[1], dif = rec[3];
  SurfVtx v;
  v.pos = mk(p.x, p.y, p.z);
  v.N = mk(nr.x, nr.y, nr.z);
  v.dif = mk(dif.x, dif.y, dif.z);
  v.spec = mk(0);
  v.rough = 0.0f;
  v.isSpec = false;
  if (GGX) {
    const float4 sp = rec[4];
    v.spec = mk(sp.x, sp.y, sp.z);
    v.rough = nr.w * nr.w;  // shadeHit's roughness from linearRoughness
    v.isSpec = specular && specular[i] != 0;
  }
  return v;
}
// the direction from a vertex to its predecessor: normalize(prev - pos) as gen_connect forms woE / woL, or the record's V
template <bool GGX>
__device__ __forceinline__ f3 outgoing(const float4* rec, const float4* prev, uint32_t i, f3 pos) {
  if (!GGX) return mk(0);  // (never read)
  if (prev) {
    const float4 q = prev[i];
    return normalize(mk(q.x, q.y, q.z) - pos);
  }
  const float4 v = rec[2];
  return mk(v.x, v.y, v.z);
}
}  // namespace

// bdpt_connect_sample: three float4 per item, (org, tmin) (dir, tmax) (value, status)
template <bool GGX, bool COMPACT>
__global__ __launch_bounds__(kWave) void connect_vertices_kernel(ConnectQueryDev Q) {
  BDPT_ONE_WAVE_PER_GROUP();
  uint32_t i, n;
  if (queryLanePast<COMPACT>(Q.range.cap, Q.range.count, i, n)) return;
  bool emit = false;
  float4 q0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), q1 = q0;
  if (i < n) {
    const float4* er = Q.eye + (size_t)i * 6;
    const float4* lr = Q.light + (size_t)i * 6;
    const SurfVtx ev = loadSurfVtx<GGX>(er, Q.eyeSpecular, i), le = loadSurfVtx<GGX>(lr, Q.lightSpecular, i);
    // the ray is formed from the two positions whatever prim says (the pass traces such rays in its lazy rounds)
    f3 dirAB;
    float lengthAB;
    pairRay(ev.pos, le.pos, dirAB, lengthAB);
    f3 value = mk(0);
    if (__float_as_int(er[5].w) >= 0 && __float_as_int(lr[5].w) >= 0)
      pairValue<GGX>(ev, outgoing<GGX>(er, Q.eyePrev, i, ev.pos), le, outgoing<GGX>(lr, Q.lightPrev, i, le.pos), value);
    emit = !allZero(value);
    q0 = make_float4(ev.pos.x, ev.pos.y, ev.pos.z, Q.range.minT);
    q1 = make_float4(dirAB.x, dirAB.y, dirAB.z, lengthAB);
    float4* o = Q.out + (size_t)i * 3;
    o[0] = q0;
    o[1] = q1;
    o[2] = make_float4(value.x, value.y, value.z, __uint_as_float(emit ? BDPT_CONNECT_STATUS_NONZERO : 0u));
  }
  if (COMPACT) compactAppend(Q.compact, Q.range.cap, emit, i, q0, q1);
}

// bdpt_camera_sample: four float4 per item, (org, tmin) (dir, tmax) (f, G) (pixel, status, 0, 0)
template <bool GGX, bool COMPACT>
__global__ __launch_bounds__(kWave) void connect_camera_kernel(ConnectQueryDev Q, bdpt_camera camera) {
  BDPT_ONE_WAVE_PER_GROUP();
  uint32_t i, n;
  if (queryLanePast<COMPACT>(Q.range.cap, Q.range.count, i, n)) return;
  bool emit = false;
  float4 q0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), q1 = q0;
  if (i < n) {
    const float4* lr = Q.light + (size_t)i * 6;
    float4 q2 = q0;
    uint32_t pixel = 0xffffffffu, status = 0u;
    if (__float_as_int(lr[5].w) >= 0) {
      const SplatCam cam = splatCam(camera);
      const SurfVtx lv = loadSurfVtx<GGX>(lr, Q.lightSpecular, i);
      const f3 dirToCamera = normalize(cam.pos - lv.pos);
      const float disToCamera = length(cam.pos - lv.pos);
      float fx = 0.0f, fy = 0.0f;
      if (splatTarget(cam, dirToCamera, Q.width, Q.height, Q.jitter[0], Q.jitter[1], fx, fy)) {
        f3 vV = mk(0);
        if (GGX) {
          const float4 v = lr[2];  // the walk's stored F_V plane
          vV = mk(v.x, v.y, v.z);
        }
        f3 fr;
        float Gt;
        splatTerm<GGX>(cam, lv, vV, dirToCamera, disToCamera, fr, Gt);
        pixel = (uint32_t)fx + (uint32_t)fy * Q.width;
        status = BDPT_CONNECT_STATUS_PIXEL | ((!allZero(fr) && Gt != 0.0f) ? BDPT_CONNECT_STATUS_NONZERO : 0u);
        q2 = make_float4(fr.x, fr.y, fr.z, Gt);
        emit = true;  // the pass traces it whatever its value: a zero-valued splat still saturates its pixel
      }
      q0 = make_float4(lv.pos.x, lv.pos.y, lv.pos.z, Q.range.minT);
      q1 = make_float4(dirToCamera.x, dirToCamera.y, dirToCamera.z, disToCamera);
    }
    float4* o = Q.out + (size_t)i * 4;
    o[0] = q0;
    o[1] = q1;
    o[2] = q2;
    o[3] = make_float4(__uint_as_float(pixel), __uint_as_float(status), 0.0f, 0.0f);
  }
  if (COMPACT) compactAppend(Q.compact, Q.range.cap, emit, i, q0, q1);
}

// Entry j uses item k = items ? items[j] : j: pixels[k], values[k], visible[j].  64-bit vector atomics on integers: the
// sums are exact whatever the order.
__global__ __launch_bounds__(kWave) void splat_add_kernel(SplatAddDev A) {
  BDPT_ONE_WAVE_PER_GROUP();
  uint32_t j;
  if (queryLanePast(A.cap, A.count, j)) return;
  if (A.visible && A.visible[j] == 0) return;
  const uint32_t k = A.items ? A.items[j] : j;
  const uint32_t pix = A.pixels[k];
  if (pix >= A.numPixels) return;
  const float4 c = A.values[k];
  unsigned long long* sp = A.splat + (size_t)pix * 4;
  // a NaN or non-positive channel adds nothing (gatherLane's terms are clamped, hence never negative)
  const unsigned long long qx = c.x > 0.0f ? toFixed(c.x) : 0ull, qy = c.y > 0.0f ? toFixed(c.y) : 0ull,
                           qz = c.z > 0.0f ? toFixed(c.z) : 0ull;
  if (qx) atomicAdd(&sp[0], qx);
  if (qy) atomicAdd(&sp[1], qy);
  if (qz) atomicAdd(&sp[2], qz);
  atomicAdd(&sp[3], 1ull);
}

void launchConnectQuery(const ConnectQueryDev& Q, const bdpt_camera* cam, bool ggx, hipStream_t st) {
  if (!Q.range.cap) return;
  const uint32_t g = wavesFor(Q.range.cap);
  withFlag(ggx, [&](auto GGX) {
    withFlag(Q.compact.rays != nullptr, [&](auto COMPACT) {
      if (cam)
        launchWave(connect_camera_kernel<GGX, COMPACT>, g, st, Q, *cam);
      else
        launchWave(connect_vertices_kernel<GGX, COMPACT>, g, st, Q);
    });
  });
}

void launchSplatAdd(const SplatAddDev& A, hipStream_t st) {
  if (!A.cap) return;
  launchWave(splat_add_kernel, wavesFor(A.cap), st, A);
}

}  // namespace bdpt
