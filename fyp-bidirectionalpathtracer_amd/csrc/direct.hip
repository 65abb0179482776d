// direct.hip — bdpt_direct_query and bdpt_direct_execute: direct lighting from every light of the scene, one any-hit ray
// per (item, light) that can change the result, from one persistent kernel.
//
// Replaces the reference's Lambertian-plus-shadows pass (CommonPasses/Data/CommonPasses/lambertianPlusShadows.rt.hlsl:
// 51-149 — the ray generation shader's loop over the lights with its shadow any-hit / miss pair — driven by
// CommonPasses/LambertianPlusShadowPass.cpp:64-83), and the loop a caller otherwise runs per light: bdpt_set_lights with a
// one-light table -> bdpt_light_query(NEE) -> bdpt_trace_rays(BDPT_TRACE_ANY) -> an accumulate.
//
// Built on the item loop of device_item_loop.hpp through its helpers: feedInit / refill, nodePhase, leafPhase, parkedDue and
// releaseCursor are called, none of the loop is kept as the kernel's own text: with the fetch and both phases written out
// as ao.hip has them the kernel took 3 more VGPRs and measured the same (DESIGN.md "Direct lighting").  What is
// its own is what a lane without a ray in flight does — at fetch and after each answer alike, so the text exists once:
// it walks k forward over the lights (at most BDPT_MAX_LIGHTS iterations, which may diverge), adds the terms that need
// no ray (LdotN == 0, or an intensity of all +-0), settles the ones the light's cube map of occluder hints answers
// (HINTS: point and spot lights, recOccludes on lightHint's triangle, as light_query.hip tries it), and either starts
// light k's ray in its own slot (travInit from the kept origin, TravState::o) or retires with one store per output.
// No output atomics: every output word has one writer, whatever the order the lanes run in.  Dead items never take a
// slot: their outputs are written at fetch.
//
// Termination: k only grows while a lane holds its item, each k traces at most one ray, and a traversal is finite, so an
// item retires after at most numLights <= 16 rays.  The wave leaves when the cursor is exhausted and no lane holds an item.
//
// Across a traversal a lane keeps its item, k, the two masks (one register), the answer, the sum, and with
// BDPT_DIRECT_KEEP_TERM N, LdotN and I of the ray in flight; without it N is re-read from the record and getLightData runs
// again for light k when the answer comes (same inputs, same bits).  The diffuse colour is read when the item retires.
// The item itself, a record or a G-buffer pixel, is read and written through device_item_source.hpp.
#include "kernels.h"

#include "device_item_loop.hpp"
#include "device_item_source.hpp"
#include "device_math.hpp"
#include "device_query.hpp"
#include "device_scene.hpp"
#include "launch.hpp"

namespace bdpt {

// 1: N, LdotN and I of the ray in flight stay in seven registers across the traversal; 0: N is re-read from the record
// and the light's term is computed again when the answer comes: 82 to 88 VGPRs against 89 to 92, both five waves per SIMD,
// and 4.35 / 4.48 ms against 3.96 / 3.96 ms with 16 lights (DESIGN.md "Direct lighting"): kept ships.
#ifndef BDPT_DIRECT_KEEP_TERM
#define BDPT_DIRECT_KEEP_TERM 1
#endif
// Lanes without a ray in flight — fresh items and answered rays — walk on right after the leaf phase (1), or wait
// ("parked", as BDPT_WALKQ_SHADE_MIN of walk_query.hip) until this many of the wave wait or no lane is traversing, so that
// getLightData (two normalisations, a division, the cone's acos: a few hundred instructions) runs for many lanes at once.
// Measured with tools/direct_times.py --fused-only (DESIGN.md "Direct lighting"; 1080p atrium, two alternating runs per
// build), 16 lights: 1, 8, 16, 32 waiting lanes give 4.07 / 4.12, 4.00 / 3.99, 3.77 / 3.83, 3.65 / 3.69 ms without hints and
// 4.40 / 4.43, 4.29 / 4.31, 3.87 / 3.88, 3.68 / 3.76 ms with them; with 1 and 3 lights all four lie within one build's spread.
#ifndef BDPT_DIRECT_ADVANCE_MIN
#define BDPT_DIRECT_ADVANCE_MIN 32
#endif
// Waves per SIMD the register allocation aims for (experiment knob, as BDPT_AO_WAVES_PER_EU of ao.hip): 5 is what the kernel
// needs without spilling (90 VGPRs without hints, 93 with; 4 gives the same code).  At 6 (80 VGPRs) the allocator spills 56
// to 64 bytes per lane to scratch, which the kernel must not use.
#ifndef BDPT_DIRECT_WAVES_PER_EU
#define BDPT_DIRECT_WAVES_PER_EU 5
#endif

namespace {

// item `i`: the colour the sum is multiplied by: diffuse, or specular where diffuse is (nearly) black
// (lambertianPlusShadows.rt.hlsl:109-114)
template <int SRC>
__device__ __forceinline__ f3 directAlbedo(const DirectDev& Q, uint32_t i) {
  f3 dif = itemDiffuse<SRC>(Q, i), spec;
  if (SRC == ITEM_SRC_SURFACES) {
    const float4 q4 = Q.surf[(size_t)i * 6 + 4];
    spec = mk(q4.x, q4.y, q4.z);
  } else {
    spec = itemHalf3(Q.gbSpecRough, Q.pix[i]);
  }
  if (dot(dif, dif) < 0.00001f) dif = spec;
  return dif;
}

// the outputs of item `i`; masks: bits 0-15 `visible`, bits 16-31 `traced`
template <int SRC>
__device__ __forceinline__ void directStore(const DirectDev& Q, uint32_t i, f3 color, uint32_t masks) {
  itemStoreColor<SRC>(Q, i, color);
  if (SRC == ITEM_SRC_SURFACES) {
    if (Q.visible) Q.visible[i] = masks & 0xffffu;
    if (Q.traced) Q.traced[i] = masks >> 16;
  }
}

}  // namespace

// cursor: as releaseCursor has it (both words zero when a launch starts and when it ends).
template <int SRC, bool HINTS>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(BDPT_DIRECT_WAVES_PER_EU, 8))) void direct_kernel(
    SceneDev S, DirectDev Q, unsigned long long* cursor) {
  BDPT_ONE_WAVE_PER_GROUP();
  __shared__ int s_stack[kStackLds * kWave];
  int* stk = s_stack + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const uint32_t numLights = S.numLights < (uint32_t)BDPT_MAX_LIGHTS ? S.numLights : (uint32_t)BDPT_MAX_LIGHTS;  // k < 16: the masks' shifts
  ItemFeed F = feedInit(itemCount(Q.range.cap, Q.range.count));
  bool has = false, flying = false;  // flying: the lane's ray toward light k is in flight
  uint32_t rid = 0, k = 0, masks = 0;
  int answer = -1;  // of the ray toward light k: -1 none (yet), 0 it is occluded, 1 it is not
  f3 sum = mk(0);
#if BDPT_DIRECT_KEEP_TERM
  f3 keptN = mk(0), keptI = mk(0);
  float keptLdotN = 0.0f;
#endif
  TravState T;
  T.cur = kDone;
  T.o = mk(0);
  T.best.prim = -1;
  while (refill(F, cursor, lane, has, [&](uint32_t item) {
    f3 pos = mk(0);
    if (!itemAlive<SRC>(Q, item, pos)) {
      directStore<SRC>(Q, item, directAlbedo<SRC>(Q, item), 0u);  // the background branch: (colour, 1); the lane stays idle
      return;
    }
    rid = item;
    k = 0;
    masks = 0;
    sum = mk(0);
    T.o = pos;  // the origin of every ray of the item
#if BDPT_DIRECT_KEEP_TERM
    keptN = itemNormal<SRC>(Q, item);
#endif
    flying = false;
    answer = -1;
    has = true;
  })) {
    const bool leavesDue = nodePhase<0>(S, T, stk, flying);
    if (leavesDue && flying && T.cur < 0 && leafPhase<BDPT_TRACE_ANY>(S, T, stk)) {
      flying = false;
      answer = (T.best.prim < 0) ? 1 : 0;
      T.cur = kDone;
    }
    if (parkedDue<BDPT_DIRECT_ADVANCE_MIN>(has && !flying, flying) && has && !flying) {
      // the walk over the lights: from light k with its answer, or from a fresh item's light 0
      const f3 pos = T.o;
#if BDPT_DIRECT_KEEP_TERM
      const f3 N = keptN;
#else
      const f3 N = itemNormal<SRC>(Q, rid);
#endif
      while (k < numLights) {
        const bdpt_light& lt = S.sc->lights[k];
        f3 L = mk(0), I;
        float LdotN, dist = 0.0f;
#if BDPT_DIRECT_KEEP_TERM
        if (answer >= 0) {
          I = keptI;
          LdotN = keptLdotN;
        } else
#endif
        {
          getLightData(lt, pos, L, I, dist);
          LdotN = saturate(dot(N, L));
        }
        // no ray where it cannot change a bit: (0 * LdotN) * I and (1 * LdotN) * I are the same
        const bool need = LdotN != 0.0f && !allZero(I);
        float s = 1.0f;
        if (need && answer < 0) {
          masks |= 0x10000u << k;
          const f3 term = LdotN * I;
          const bool positive = term.x > 0.0f || term.y > 0.0f || term.z > 0.0f;
          if (HINTS && positive && lt.type != BDPT_LIGHT_DIRECTIONAL &&
              recOccludes(S, lightHint(S, (int)k, ld3(lt.posW), pos), pos, L, Q.range.minT, dist)) {
            s = 0.0f;  // the light's nearest triangle toward the item occludes the segment: no traversal
          } else {
            travInit(T, pos, L, Q.range.minT, dist);  // the lane keeps its slot
#if BDPT_DIRECT_KEEP_TERM
            keptI = I;
            keptLdotN = LdotN;
#endif
            flying = true;
            break;
          }
        } else if (need) {
          s = (float)answer;
        }
        answer = -1;
        sum = sum + (s * LdotN) * I;  // lambertianPlusShadows.rt.hlsl:140, as written: a non-finite I gives its NaN or inf
        if (s != 0.0f) masks |= 1u << k;
        k++;
      }
      if (!flying) {
        directStore<SRC>(Q, rid, sum * (directAlbedo<SRC>(Q, rid) / 3.141592f), masks);  // .hlsl:144: the shader's literal
        has = false;
      }
    }
  }
  releaseCursor(cursor, lane);
}

void launchDirect(const SceneDev& S, const DirectDev& Q, bool gbuffer, bool hints, unsigned long long* cursor, LaunchGrids& G, int numCUs,
                  hipStream_t st) {
  if (!Q.range.cap) return;
  withFlag(gbuffer, [&](auto GB) {
    withFlag(hints, [&](auto HINTS) {
      launchPersistent(direct_kernel<GB ? ITEM_SRC_GBUFFER : ITEM_SRC_SURFACES, HINTS>, G.direct[(GB ? 2 : 0) + (HINTS ? 1 : 0)],
                       Q.range.cap, numCUs, st, S, Q, cursor);
    });
  });
}

}  // namespace bdpt
