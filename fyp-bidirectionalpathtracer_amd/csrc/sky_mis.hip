// sky_mis.hip — bdpt_sky_mis_query and bdpt_sky_mis_execute: sky lighting with multiple importance sampling.  Per item and
// sample one any-hit ray toward a direction drawn from the environment map's table and one toward a direction drawn from
// the BSDF (GGX or Lambertian), each weighted by the balance heuristic, from one persistent kernel.
//
// Replaces the loop a caller otherwise runs per sample: bdpt_env_query(SAMPLE) -> bdpt_bsdf_pdf_query -> glue ->
// bdpt_trace_rays(ANY) -> add, then bdpt_bsdf_query(SAMPLE) -> bdpt_env_query(EVAL) -> bdpt_bsdf_pdf_query -> glue ->
// bdpt_trace_rays(ANY) -> add (include/bdpt.h "Environment lighting" has the definition; the two are equal bit for bit).
//
// Shaped like sky_kernel (sky.hip) on the item loop of device_item_loop.hpp: a lane owns its item through all its
// 2 * samples terms L_0, B_0, L_1, B_1, ...; `techniques` (wave-uniform) leaves one kind out.  When its ray is answered the
// lane adds the term, makes its next one in its own slot — envSample and the BSDF's density toward it, or sampleBRDF,
// envEval and the density — and starts that ray; terms whose value is all +-0 trace no ray and are passed over at once.
// After the last term the lane retires with one store per output: no output atomics, every word has one writer.  Dead
// items never take a slot: their outputs are written at fetch.  Across the traversal a lane keeps its item, the term index,
// count, the RNG state, the sum and the term its ray gates; N, V, the colours and the roughness are re-read when it
// regenerates, the origin lives in the traversal state.  The item itself, a record or a G-buffer pixel, is read and
// written through device_item_source.hpp; the GGX reads (V, specular, roughness) are this file's.
#include "kernels.h"

#include "device_bsdf_pdf.hpp"
#include "device_item_loop.hpp"
#include "device_item_source.hpp"
#include "device_math.hpp"
#include "device_query.hpp"
#include "device_scene.hpp"
#include "env_light.h"
#include "launch.hpp"

namespace bdpt {

// Waves per SIMD the register allocation aims for (experiment knob, as BDPT_SKY_WAVES_PER_EU of sky.hip): DESIGN.md "MIS sky
// lighting" has the resource usage of the four instances.
#ifndef BDPT_SKY_MIS_WAVES_PER_EU
#define BDPT_SKY_MIS_WAVES_PER_EU 4
#endif
// Answered lanes wait ("parked", as BDPT_GI_SHADE_MIN of gi.hip) until this many of the wave wait, or no lane is traversing,
// so that the next terms — two table searches, or a BSDF sample and an environment lookup, plus the density — are made for
// many lanes at once.  1: never wait.  Measured with tools/sky_mis_times.py --fused-only (DESIGN.md "MIS sky lighting"; 1080p
// atrium, 32 samples, GGX): 1, 8, 16, 32, 48, 64 waiting lanes give 45.1, 43.8, 40.0, 34.5, 34.3, 38.8 ms; two runs of one
// build differ by 0.3 ms.
#ifndef BDPT_SKY_MIS_REGEN_MIN
#define BDPT_SKY_MIS_REGEN_MIN 32
#endif

namespace {

struct SkyMisShading {
  f3 N, V, dif, spec;
  float rough;
};

// item `i` at `pos`: what its BSDF reads.  The Lambertian instances read N and diffuse only.
template <int SRC, bool GGX>
__device__ __forceinline__ SkyMisShading skyMisShading(const SkyMisDev& Q, uint32_t i, f3 pos) {
  SkyMisShading sd;
  sd.V = mk(0);
  sd.spec = mk(0);
  sd.rough = 0.0f;
  sd.N = itemNormal<SRC>(Q, i);
  sd.dif = itemDiffuse<SRC>(Q, i);
  if (!GGX) return sd;
  if (SRC == ITEM_SRC_SURFACES) {
    const float4* r = Q.surf + (size_t)i * 6;
    const float4 q1 = r[1], q2 = r[2], q4 = r[4];
    sd.V = mk(q2.x, q2.y, q2.z);
    sd.spec = mk(q4.x, q4.y, q4.z);
    sd.rough = q1.w * q1.w;
  } else {  // as init_paths_kernel reads the pixel
    const uint2 raw = reinterpret_cast<const uint2*>(Q.gbSpecRough)[Q.pix[i]];
    sd.spec = mk(f16_to_f32((uint16_t)(raw.x & 0xffffu)), f16_to_f32((uint16_t)(raw.x >> 16)), f16_to_f32((uint16_t)(raw.y & 0xffffu)));
    const float a = f16_to_f32((uint16_t)(raw.y >> 16));
    sd.rough = a * a;
    sd.V = normalize(ld3(Q.camPos) - pos);
  }
  return sd;
}
// the outputs of item `i`
template <int SRC>
__device__ __forceinline__ void skyMisStore(const SkyMisDev& Q, uint32_t i, f3 color, uint32_t count, uint32_t seed) {
  itemStoreColor<SRC>(Q, i, color);
  if (SRC == ITEM_SRC_SURFACES) {
    if (Q.counts) Q.counts[i] = count;
    if (Q.seedsOut) Q.seedsOut[i] = seed;
  }
}

// The item's terms from h on, in order (h even: the table-sampled term of sample h / 2, odd: its BSDF-sampled term): a
// term whose clamped value is all +-0 is added at once (no ray); the first other one starts its ray from `pos` and is kept
// in `pend`.  Returns whether a ray is in flight; false: h == 2 * samples.
template <int SRC, bool GGX>
__device__ __forceinline__ bool skyMisNext(const SkyMisDev& Q, uint32_t i, f3 pos, uint32_t& h, uint32_t& seed, f3& sum, f3& pend,
                                           TravState& T) {
  const SkyMisShading sd = skyMisShading<SRC, GGX>(Q, i, pos);
  const bool useTable = (Q.techniques & 1u) != 0u, useBsdf = (Q.techniques & 2u) != 0u;
  const uint32_t end = 2u * Q.samples;
  while (h < end) {
    const bool bsdfTerm = (h & 1u) != 0u;
    h++;
    if (!(bsdfTerm ? useBsdf : useTable)) continue;
    f3 dir, value = mk(0);
    if (!bsdfTerm) {
      const EnvSample e = envSample(Q.table, seed);  // four draws
      dir = mk(e.dir[0], e.dir[1], e.dir[2]);
      if (e.pdf != 0.0f) {
        f3 fcos;
        float pB;
        bsdfFcosPdf<GGX>(dir, sd.N, sd.V, sd.dif, sd.spec, sd.rough, fcos, pB);
        if (!useBsdf) pB = 0.0f;
        value = clampVec((fcos * mk(e.radiance[0], e.radiance[1], e.radiance[2])) / (e.pdf + pB), Q.clampUpper);
      }
    } else {
      float pdf;
      bool isSpec;
      sampleBRDF<GGX>(seed, sd.N, sd.N, sd.V, sd.dif, sd.spec, sd.rough, false, dir, pdf, isSpec);  // the state by value
      nextRand(seed);  // three draws, whichever sampler ran
      nextRand(seed);
      nextRand(seed);
      if (pdf != 0.0f) {
        const float d[3] = {dir.x, dir.y, dir.z};
        const EnvEval ev = envEval(Q.table, d);
        f3 fcos;
        float pB;
        bsdfFcosPdf<GGX>(dir, sd.N, sd.V, sd.dif, sd.spec, sd.rough, fcos, pB);
        const float pL = useTable ? ev.pdf : 0.0f;
        value = clampVec((fcos * mk(ev.radiance[0], ev.radiance[1], ev.radiance[2])) / (pL + pB), Q.clampUpper);
      }
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
template <int SRC, bool GGX>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(BDPT_SKY_MIS_WAVES_PER_EU, 8))) void sky_mis_kernel(
    SceneDev S, SkyMisDev Q, unsigned long long* cursor) {
  BDPT_ONE_WAVE_PER_GROUP();
  __shared__ int s_stack[kStackLds * kWave];
  int* stk = s_stack + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  ItemFeed F = feedInit(itemCount(Q.range.cap, Q.range.count));
  bool has = false, parked = false;
  uint32_t rid = 0, h = 0, count = 0, seed = 0;
  f3 sum = mk(0), pend = mk(0);
  TravState T;
  T.cur = kDone;
  while (refill(F, cursor, lane, has, [&](uint32_t item) {
    rid = item;
    seed = itemSeed<SRC>(Q, rid);
    f3 pos = mk(0);
    if (!itemAlive<SRC>(Q, rid, pos)) {
      // the background: the diffuse channel holds the colour, no draw; the lane stays idle
      skyMisStore<SRC>(Q, rid, itemDiffuse<SRC>(Q, rid), 0u, seed);
    } else {
      h = 0;
      count = 0;
      sum = mk(0);
      if (skyMisNext<SRC, GGX>(Q, rid, pos, h, seed, sum, pend, T)) {
        has = true;
      } else {
        skyMisStore<SRC>(Q, rid, sum / (float)Q.samples, 0u, seed);  // no term of the item was worth a ray
      }
    }
  })) {
    const bool leavesDue = nodePhase<0>(S, T, stk, has && !parked);
    if (leavesDue && has && !parked && T.cur < 0) parked = leafPhase<BDPT_TRACE_ANY>(S, T, stk);
    if (parkedDue<BDPT_SKY_MIS_REGEN_MIN>(parked, has && !parked) && parked) {
      parked = false;
      if (T.best.prim < 0) {  // unoccluded
        sum = sum + pend;
        count++;
      }
      if (!skyMisNext<SRC, GGX>(Q, rid, T.o, h, seed, sum, pend, T)) {
        skyMisStore<SRC>(Q, rid, sum / (float)Q.samples, count, seed);
        has = false;
        T.cur = kDone;
      }
    }
  }
  releaseCursor(cursor, lane);
}

void launchSkyMis(const SceneDev& S, const SkyMisDev& Q, bool gbuffer, bool ggx, unsigned long long* cursor, LaunchGrids& G, int numCUs,
                  hipStream_t st) {
  if (!Q.range.cap) return;
  withFlag(gbuffer, [&](auto GB) {
    withFlag(ggx, [&](auto GGX) {
      launchPersistent(sky_mis_kernel<GB ? ITEM_SRC_GBUFFER : ITEM_SRC_SURFACES, GGX>, G.skyMis[(GB ? 2 : 0) + (GGX ? 1 : 0)],
                       Q.range.cap, numCUs, st, S, Q, cursor);
    });
  });
}

}  // namespace bdpt
