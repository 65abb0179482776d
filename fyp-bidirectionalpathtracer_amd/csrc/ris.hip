// ris.hip — bdpt_ris_query and bdpt_ris_execute: resampled direct lighting (resampled importance sampling, the first stage
// of ReSTIR).  Per item and sample `candidates` next-event candidates of the pass are drawn, one of them survives in a
// one-entry reservoir with probability proportional to its unshadowed contribution at the item, and one any-hit ray is
// traced for the survivor: `samples` rays per item whatever the light count, from one persistent kernel.
//
// Replaces the loop a caller otherwise runs per sample and candidate: bdpt_light_query(NEE) -> a draw -> clamp, weight and
// reservoir update, then bdpt_trace_rays(ANY) for the survivors and an ordered add (include/bdpt.h "Resampled direct
// lighting" has the definition; the two are equal bit for bit).  A candidate is lightCandidate of device_light.hpp, the
// text bdpt_light_query itself runs.
//
// Shaped like direct_kernel (direct.hip) on the item loop of device_item_loop.hpp: what a lane without a ray in flight does
// — at fetch and after each answer alike — exists once.  It makes its next sample's candidates in a loop, adds the samples
// that need no ray (nothing selected, or the light's occluder hint answers: HINTS, point and spot lights), and either
// starts the survivor's ray in its own slot or retires with one store per output.  Such lanes wait ("parked") until
// BDPT_RIS_REGEN_MIN of the wave do, or none is traversing.  No output atomics: every output word has one writer.  Dead
// items never take a slot: their outputs are written at fetch.
//
// Termination: k only grows while a lane holds its item, each k makes `candidates` candidates and traces at most one ray,
// and a traversal is finite.  The wave leaves when the cursor is exhausted and no lane holds an item.
//
// Across a traversal a lane keeps its item, k, the RNG state, the sum, the ray count, the term its ray gates and the
// reservoir record of the sample; N, V, the colours and the roughness are re-read when it regenerates, the origin lives in
// the traversal state.  The item itself, a record or a G-buffer pixel, is read and written through
// device_item_source.hpp; the GGX reads (V, specular, roughness) are this file's, as skyMisShading of sky_mis.hip has them.
#include "kernels.h"

#include "device_item_loop.hpp"
#include "device_item_source.hpp"
#include "device_light.hpp"
#include "device_math.hpp"
#include "device_query.hpp"
#include "device_scene.hpp"
#include "launch.hpp"

namespace bdpt {

// Waves per SIMD the register allocation aims for (experiment knob, as BDPT_SKY_MIS_WAVES_PER_EU of sky_mis.hip): DESIGN.md
// "Resampled direct lighting" has the resource usage of the sixteen instances.
#ifndef BDPT_RIS_WAVES_PER_EU
#define BDPT_RIS_WAVES_PER_EU 4
#endif
// ... and of the AREA instances, whose candidates also hold areaNee's emitter point
#ifndef BDPT_RIS_AREA_WAVES_PER_EU
#define BDPT_RIS_AREA_WAVES_PER_EU 3
#endif
// Lanes without a ray in flight — fresh items and answered rays — wait until this many of the wave wait, or no lane is
// traversing, so that the candidates (getLightData, directIfVisible, and for the emitter table a binary search and a
// shadeHit, each `candidates` times) are made for many lanes at once.  1: never wait.  Measured with tools/ris_times.py
// --fused-only (DESIGN.md "Resampled direct lighting"; 1080p atrium, 16 lights, one run per build, two of the 32 build within
// 1.5 %): 1, 16, 32, 48 waiting lanes give 7.82, 6.52, 5.39, 5.09 ms for 8 candidates x 8 samples (Lambertian) and 19.9, 14.8,
// 10.9, 9.59 ms for 32 x 8; with one sample 0.79, 0.76, 0.71, 0.73 and 1.72, 1.64, 1.38, 1.36 ms.  48 is slower only where
// there is little to regenerate: one candidate (0.53 against 0.47 ms at one sample) and 2 to 6 % at 4 or 8 candidates x 1.
#ifndef BDPT_RIS_REGEN_MIN
#define BDPT_RIS_REGEN_MIN 48
#endif

namespace {

constexpr uint32_t kRisNoLight = 0xffffu;  // bdpt_ris_reservoir::light of a sample that selected nothing

struct RisShading {
  f3 N, V, dif, spec;
  float rough;
};

// item `i` at `pos`: what a candidate's value reads.  The Lambertian instances read N and diffuse only.
template <int SRC, bool GGX>
__device__ __forceinline__ RisShading risShading(const RisDev& Q, uint32_t i, f3 pos) {
  RisShading sd;
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

// the reservoir record of sample `k` of item `i`: (light | status << 16, the selected state, W, wsum); a pixel's records
// lie at its place in the full frame (bdpt_ris_execute_reservoirs)
template <int SRC>
__device__ __forceinline__ void risStoreReservoir(const RisDev& Q, uint32_t i, uint32_t k, uint4 rec) {
  if (Q.reservoirs) Q.reservoirs[(size_t)(SRC == ITEM_SRC_SURFACES ? i : Q.pix[i]) * Q.samples + k] = rec;
}
// the outputs of item `i` but its reservoir records
template <int SRC>
__device__ __forceinline__ void risStore(const RisDev& Q, uint32_t i, f3 color, uint32_t traced, uint32_t seed) {
  itemStoreColor<SRC>(Q, i, color);
  if (SRC == ITEM_SRC_SURFACES) {
    if (Q.traced) Q.traced[i] = traced;
    if (Q.seedsOut) Q.seedsOut[i] = seed;
  }
}

// The item's samples from k on: a sample that selects nothing, or whose survivor the light's hint finds occluded, adds +0
// and stores its reservoir record at once (no ray); the first other one starts its ray from `pos`, keeps its term in
// `pend` and its record (status bit 0 set) in `res`.  Returns whether a ray is in flight; false: k == samples.
template <int SRC, bool GGX, bool AREA, bool HINTS>
__device__ __forceinline__ bool risNext(const SceneDev& S, const RisDev& Q, const AreaDev& A, uint32_t i, f3 pos, uint32_t& k,
                                        uint32_t& seed, f3& pend, uint4& res, TravState& T) {
  const RisShading sd = risShading<SRC, GGX>(Q, i, pos);
  float areaW;
  const int lightsCount = lightsCountOf<AREA>(S, A, areaW);
  const uint32_t M = Q.candidates;
  while (k < Q.samples) {
    float wsum = 0.0f, wSel = 0.0f;
    f3 vSel = mk(0);
    LightCandidate sel;
    sel.light = -1;
    sel.area = false;
    sel.L = mk(0);
    sel.dist = 0.0f;
    uint32_t stateSel = 0;
    for (uint32_t c = 0; c < M; c++) {
      const float r = nextRand(seed);
      const uint32_t state = seed;
      LightCandidate cand;
      const f3 value = lightCandidate<GGX, AREA>(S, A, areaW, lightsCount, r, state, pos, sd.N, sd.V, sd.dif, sd.spec, sd.rough, cand);
      const float u = nextRand(seed);
      const f3 v = clampVec(value, Q.clampUpper);
      const float w = maxf(maxf(v.x, v.y), v.z);
      wsum = wsum + w;
      if (w > 0.0f && u * wsum <= w) {
        vSel = v;
        wSel = w;
        sel = cand;
        stateSel = state;
      }
    }
    const uint32_t kk = k++;
    if (sel.light < 0) {
      risStoreReservoir<SRC>(Q, i, kk, make_uint4(kRisNoLight, 0u, 0u, __float_as_uint(wsum)));
      continue;
    }
    const float W = (wsum / (float)M) / wSel;
    const f3 term = vSel * W;
    uint32_t word = (uint32_t)sel.light | (BDPT_RIS_STATUS_RAY << 16);
    if (HINTS) {
      const bool positive = term.x > 0.0f || term.y > 0.0f || term.z > 0.0f;
      if (positive && !sel.area && S.sc->lights[sel.light].type != BDPT_LIGHT_DIRECTIONAL &&
          recOccludes(S, lightHint(S, sel.light, ld3(S.sc->lights[sel.light].posW), pos), pos, sel.L, Q.range.minT, sel.dist)) {
        // the light's nearest triangle toward the item occludes the segment: no traversal, the term counts as +0
        risStoreReservoir<SRC>(Q, i, kk, make_uint4(word | (BDPT_RIS_STATUS_HINT_OCCLUDED << 16), stateSel, __float_as_uint(W), __float_as_uint(wsum)));
        continue;
      }
    }
    pend = term;
    res = make_uint4(word, stateSel, __float_as_uint(W), __float_as_uint(wsum));
    travInit(T, pos, sel.L, Q.range.minT, sel.dist);  // the lane keeps its slot
    return true;
  }
  return false;
}

}  // namespace

// cursor: as releaseCursor has it (both words zero when a launch starts and when it ends).
template <int SRC, bool GGX, bool AREA, bool HINTS>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(AREA ? BDPT_RIS_AREA_WAVES_PER_EU : BDPT_RIS_WAVES_PER_EU, 8))) void ris_kernel(
    SceneDev S, RisDev Q, AreaDev A, unsigned long long* cursor) {
  BDPT_ONE_WAVE_PER_GROUP();
  __shared__ int s_stack[kStackLds * kWave];
  int* stk = s_stack + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  ItemFeed F = feedInit(itemCount(Q.range.cap, Q.range.count));
  bool has = false, flying = false;  // flying: the lane's ray for sample k - 1 is in flight
  uint32_t rid = 0, k = 0, seed = 0, traced = 0;
  f3 sum = mk(0), pend = mk(0);
  uint4 res = make_uint4(0u, 0u, 0u, 0u);
  TravState T;
  T.cur = kDone;
  T.o = mk(0);
  T.best.prim = -1;
  while (refill(F, cursor, lane, has, [&](uint32_t item) {
    f3 pos = mk(0);
    if (!itemAlive<SRC>(Q, item, pos)) {
      // the background: the diffuse channel holds the colour, no draw, no selection; the lane stays idle.  Only a record's
      // state is stored (unchanged); a pixel's initRand is not made for nothing.
      risStore<SRC>(Q, item, itemDiffuse<SRC>(Q, item), 0u, SRC == ITEM_SRC_SURFACES ? itemSeed<SRC>(Q, item) : 0u);
      if (SRC == ITEM_SRC_SURFACES && Q.reservoirs)  // (a background pixel's records are not written: no stage reads them)
        for (uint32_t j = 0; j < Q.samples; j++) risStoreReservoir<SRC>(Q, item, j, make_uint4(kRisNoLight, 0u, 0u, 0u));
      return;
    }
    rid = item;
    k = 0;
    seed = itemSeed<SRC>(Q, item);
    traced = 0;
    sum = mk(0);
    T.o = pos;  // the origin of every ray of the item
    flying = false;
    has = true;
  })) {
    const bool leavesDue = nodePhase<0>(S, T, stk, flying);
    if (leavesDue && flying && T.cur < 0 && leafPhase<BDPT_TRACE_ANY>(S, T, stk)) {
      flying = false;
      if (T.best.prim < 0)
        sum = sum + pend;  // unoccluded
      else
        res.x |= BDPT_RIS_STATUS_OCCLUDED << 16;
      risStoreReservoir<SRC>(Q, rid, k - 1u, res);
      T.cur = kDone;
    }
    if (parkedDue<BDPT_RIS_REGEN_MIN>(has && !flying, flying) && has && !flying) {
      if (risNext<SRC, GGX, AREA, HINTS>(S, Q, A, rid, T.o, k, seed, pend, res, T)) {
        flying = true;
        traced++;
      } else {
        risStore<SRC>(Q, rid, sum / (float)Q.samples, traced, seed);
        has = false;
        T.cur = kDone;
      }
    }
  }
  releaseCursor(cursor, lane);
}

void launchRis(const SceneDev& S, const RisDev& Q, const AreaDev& A, bool gbuffer, bool ggx, bool hints, unsigned long long* cursor,
               LaunchGrids& G, int numCUs, hipStream_t st) {
  if (!Q.range.cap) return;
  withFlag(gbuffer, [&](auto GB) {
    withFlag(ggx, [&](auto GGX) {
      withFlag(A.n != 0, [&](auto AREA) {
        withFlag(hints, [&](auto HINTS) {
          launchPersistent(ris_kernel<GB ? ITEM_SRC_GBUFFER : ITEM_SRC_SURFACES, GGX, AREA, HINTS>,
                           G.ris[(GB ? 8 : 0) + (GGX ? 4 : 0) + (AREA ? 2 : 0) + (HINTS ? 1 : 0)], Q.range.cap, numCUs, st, S, Q, A, cursor);
        });
      });
    });
  });
}

}  // namespace bdpt
