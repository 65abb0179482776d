// gi.hip — bdpt_gi_query and bdpt_gi_execute: direct light plus one diffuse bounce per item, up to three rays, from one
// persistent kernel.
//
// Replaces the reference's one-bounce path tracer (CommonPasses/Data/CommonPasses/simpleDiffuseGI.rt.hlsl:133-198 — the
// ray generation shader with its shadow pair and IndirectMiss / IndirectClosestHit, lines 61-108 — driven by
// CommonPasses/SimpleDiffuseGIPass.cpp:89-117), and the loop a caller otherwise runs: bdpt_light_query(NEE) ->
// bdpt_trace_rays(ANY) -> bdpt_bsdf_query(SAMPLE) -> bdpt_trace_rays(CLOSEST) -> bdpt_shade_hits -> bdpt_light_query(NEE)
// -> bdpt_trace_rays(ANY) with glue between them.
//
// Built on the item loop of device_item_loop.hpp: nodePhase, parkedDue and releaseCursor are called; the fetch (refill)
// and the leaf step are kept as the kernel's own text, the leaf step because it serves two ray types, and both because
// with them the device code is what it was before the helpers existed, and through the helpers it measured 1.3 % slower
// (DESIGN.md "The shared item loop").  A change to the fetch is made there and here.  A lane owns its item through its
// rays, phase by phase:
//   phase 0  the any-hit ray toward the light chosen for the item            -> direct
//   phase 1  the closest-hit bounce ray (BDPT_GI_INDIRECT)                   -> environment, or the shaded hit's NEE term
//   phase 2  the any-hit ray from the bounce hit toward its light            -> bounce
// and retires with one store per output: no output atomics, every word has one writer, whatever the order the lanes run
// in.  A term whose value is all +-0 traces no ray: the lane is handed on as answered "unoccluded" (T.cur = kDone).
//
// The wave holds lanes of both ray types.  An any-hit answer is an OR over the scene's triangles and a closest hit is a
// minimum with a tie rule on the triangle index, so neither depends on the order children are entered in: ONE node burst
// (nearest first, the closest-hit order) serves every lane, and the leaf phase runs the any-hit and the closest-hit
// leafStep one after the other under their masks, each skipped when no lane of the wave wants it.
//
// Termination: `phase` only grows (0 -> 1 -> 2), each phase traces at most one ray, and a traversal is finite, so an item
// retires after at most three rays; a lane whose ray is answered is advanced as soon as no lane is traversing, whatever
// the parking threshold.  The wave leaves when the cursor is exhausted and no lane holds an item.
//
// Across traversals a lane keeps its item, its phase and status bits, the RNG state, NdotL, `direct` and `pend` (the value
// the ray in flight gates); origin and direction live in the traversal state (TravState::o, ::d).  N is used up when the
// bounce direction is drawn; diffuse is re-read from the record when the item retires.  The item itself, a record or a
// G-buffer pixel, is read and written through device_item_source.hpp (itemLoad: position and normal in one body).
#include "kernels.h"

#include "device_item_loop.hpp"
#include "device_item_source.hpp"
#include "device_math.hpp"
#include "device_query.hpp"
#include "device_scene.hpp"
#include "launch.hpp"

namespace bdpt {

// Lanes whose bounce ray hit wait ("parked", as BDPT_WALKQ_SHADE_MIN of walk_query.hip) until this many of the wave wait,
// or no lane is traversing: hit shading is about a thousand instructions.  Lanes whose answer needs no shading (a shadow
// ray, a bounce that missed) advance right after the leaf phase.  Measured with tools/gi_times.py --fused-only (DESIGN.md
// "Diffuse GI"; 1080p atrium, one bounce): 1, 8, 16, 32 waiting lanes give 2.014, 1.755, 1.663, 1.671 ms; two runs of the
// 16 build 1.663 and 1.652.
#ifndef BDPT_GI_SHADE_MIN
#define BDPT_GI_SHADE_MIN 16
#endif
// Waves per SIMD the register allocation aims for (experiment knob, as BDPT_WALKQ_WAVES_PER_EU of walk_query.hip): 4 is
// what the kernel needs without spilling (105 / 108 / 110 VGPRs for the three instances; 3 gives the same code).  At 5
// (96 VGPRs) the allocator spills 52 to 68 bytes per lane to scratch, which the kernel must not use; that build measured
// 1.617 ms with the bounce against 1.663 and 0.481 against 0.449 ms direct only.
#ifndef BDPT_GI_WAVES_PER_EU
#define BDPT_GI_WAVES_PER_EU 4
#endif

// 1: diffuse is re-read from the record when the item retires, 0: it stays in three registers across the traversals (N is
// used up when the item is fetched either way).  Held: 109 / 112 / 114 VGPRs and 1.637 ms with the bounce against 1.663 re-read,
// about the spread of two runs of one build (1.663, 1.652): re-read ships.
#ifndef BDPT_GI_RELOAD_DIFFUSE
#define BDPT_GI_RELOAD_DIFFUSE 1
#endif

namespace {

// the outputs of item `i`
template <int SRC>
__device__ __forceinline__ void giStore(const GiDev& Q, uint32_t i, f3 color, uint32_t status, uint32_t seed) {
  itemStoreColor<SRC>(Q, i, color);
  if (SRC == ITEM_SRC_SURFACES) {
    if (Q.status) Q.status[i] = status;
    if (Q.seedsOut) Q.seedsOut[i] = seed;
  }
}
// the bounce ray's bdpt_hit as trace_rays_kernel writes one; giStoreNoHit: there was no bounce ray
__device__ __forceinline__ void giStoreHit(const GiDev& Q, uint32_t i, const Hit& h) {
  if (!Q.hits) return;
  const bool hit = h.prim >= 0;
  Q.hits[i] = make_float4(hit ? h.t : 0.0f, hit ? h.u : 0.0f, hit ? h.v : 0.0f, __int_as_float(h.prim));
}
__device__ __forceinline__ void giStoreNoHit(const GiDev& Q, uint32_t i) {
  if (Q.hits) Q.hits[i] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
}

// The light part of a NEE term at (pos, N, dif): bdpt_light_query(BDPT_LIGHT_NEE, matIndex 1, flags 0) — lightNeeLane of
// light_query.hip without the emitter table and hints.  One draw.  Returns the value; the ray is (pos, minT, L, dist).
__device__ __forceinline__ f3 giNee(const SceneDev& S, uint32_t& seed, f3 pos, f3 N, f3 dif, f3& L, float& distToLight) {
  const int lightsCount = (int)S.numLights;
  const float r = nextRand(seed);
  int lightToSample = (int)(r * (float)lightsCount);
  if (lightToSample > lightsCount - 1) lightToSample = lightsCount - 1;
  f3 lightIntensity;
  getLightData(S.sc->lights[lightToSample], pos, L, lightIntensity, distToLight);
  return directIfVisible<false>((float)lightsCount, L, lightIntensity, N, mk(0), dif, mk(0), 0.0f);
}

// the ray that gates `value`, or for a value of +-0 no ray: the lane is answered at once, unoccluded
__device__ __forceinline__ void giShadowRay(TravState& T, f3 value, f3 pos, f3 L, float minT, float dist) {
  travInit(T, pos, L, minT, dist);
  if (allZero(value)) T.cur = kDone;
}

// the item retires: color = direct + the bounce term as the shader writes it (simpleDiffuseGI.rt.hlsl:183-192)
template <int SRC>
__device__ __forceinline__ void giRetire(const GiDev& Q, uint32_t i, bool indirect, f3 direct, f3 bounce, float NdotL, f3 dif, uint32_t status,
                                         uint32_t seed) {
  f3 color = direct;
  if (indirect) {
    const float prob = (Q.flags & BDPT_GI_UNIFORM) ? 1.0f / (2.0f * kPi) : NdotL / kPi;
    color = direct + (((NdotL * bounce) * dif) / kPi) / prob;
  }
  giStore<SRC>(Q, i, color, status, seed);
}

}  // namespace

// cursor: as releaseCursor has it (both words zero when a launch starts and when it ends).
template <int SRC, bool NMAP>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(BDPT_GI_WAVES_PER_EU, 8))) void gi_kernel(
    SceneDev S, GiDev Q, unsigned long long* cursor) {
  BDPT_ONE_WAVE_PER_GROUP();
  __shared__ int s_stack[kStackLds * kWave];
  int* stk = s_stack + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  // refill (device_item_loop.hpp), as this kernel's own text: see the head of the file
  const uint32_t n = itemCount(Q.range.cap, Q.range.count);
  const uint32_t share = (n / gridDim.x + kWave - 1) & ~(uint32_t)(kWave - 1);
  const uint32_t chunk = share < (uint32_t)kWave ? (uint32_t)kWave : (share > kFetchChunk ? kFetchChunk : share);
  const bool indirect = (Q.flags & BDPT_GI_INDIRECT) != 0;
  bool has = false, exhausted = false, parked = false;
  uint32_t rid = 0, seed = 0, chunkPos = 0, chunkEnd = 0;
  uint32_t phase = 0, status = 0;  // phase: 0, 1, 2 — it only grows while the lane holds its item
  uint32_t nTris = 0, nAlpha = 0;  // (leafStep's tallies: not kept)
  float NdotL = 0.0f;
  f3 direct = mk(0), pend = mk(0);
#if !BDPT_GI_RELOAD_DIFFUSE
  f3 keptDif = mk(0);
#endif
  TravState T;
  T.cur = kDone;
  for (;;) {
    const unsigned long long idleMask = __ballot(!has);
    const int idle = __popcll(idleMask);
    if (!exhausted && idle >= kRefillIdle) {
      if (chunkPos >= chunkEnd) {  // wave-uniform: take a new chunk
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(cursor, (unsigned long long)chunk);
        base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(base >> 32)) << 32) |
               (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
        if (base < n) {
          chunkPos = (uint32_t)base;
          chunkEnd = (base + chunk < n) ? (uint32_t)(base + chunk) : n;
        } else {
          exhausted = true;
        }
      }
      if (!exhausted) {
        const uint32_t avail = chunkEnd - chunkPos;
        const uint32_t take = ((uint32_t)idle < avail) ? (uint32_t)idle : avail;
        const uint32_t rank = (uint32_t)__popcll(idleMask & ((1ull << lane) - 1ull));
        if (!has && rank < take) {
          rid = chunkPos + rank;
          seed = itemSeed<SRC>(Q, rid);
          f3 pos = mk(0), N = mk(0);
          if (!itemLoad<SRC, true>(Q, rid, pos, N)) {
            // the background branch: the diffuse channel holds the colour, no draw; the lane stays idle
            giStore<SRC>(Q, rid, itemDiffuse<SRC>(Q, rid), 0u, seed);
            giStoreNoHit(Q, rid);
          } else {
            phase = 0;
            status = 0;
            f3 L;
            float dist;
            const f3 dif = itemDiffuse<SRC>(Q, rid);
#if !BDPT_GI_RELOAD_DIFFUSE
            keptDif = dif;
#endif
            pend = giNee(S, seed, pos, N, dif, L, dist);
            giShadowRay(T, pend, pos, L, Q.range.minT, dist);
            if (indirect) {
              // N is used up here: the bounce direction's two draws follow the term's one (.hlsl:176-183)
              const f3 dir = (Q.flags & BDPT_GI_UNIFORM) ? getUniformHemisphereSample(seed, N) : getCosHemisphereSample(seed, N);
              NdotL = saturate(dot(N, dir));
              direct = dir;  // kept in `direct`'s registers until phase 0 is answered
            }
            has = true;
          }
        }
        chunkPos += take;
      }
    }
    if (__ballot(has) == 0ull) {
      if (exhausted) break;  // every lane retired and nothing left to take
      continue;              // (a chunk of dead items: take the next)
    }
    const bool leavesDue = nodePhase<1>(S, T, stk, has && !parked);
    if (leavesDue) {
      // the any-hit lanes' leaves, then the closest-hit lanes' (a branch no lane of the wave takes is jumped over)
      const bool atLeaf = has && !parked && T.cur < 0;
      bool finished = atLeaf && T.cur == kDone;
      if (atLeaf && !finished && phase != 1u) finished = leafStep<BDPT_TRACE_ANY, false>(S, T, nTris, nAlpha);
      if (atLeaf && !finished && phase == 1u) finished = leafStep<BDPT_TRACE_CLOSEST, false>(S, T, nTris, nAlpha);
      if (atLeaf && !finished) {
        T.cur = travPop<kStackLds>(S, T, stk);
        finished = (T.cur == kDone);
      }
      if (atLeaf) parked = finished;
    }
    // answered lanes that need no shading: a shadow ray (phase 0 or 2), or a bounce ray that missed
    if (parked && !(phase == 1u && T.best.prim >= 0)) {
      parked = false;
      const bool occluded = T.best.prim >= 0;
      bool retire = true;
      f3 bounce = mk(0);
      if (phase == 0u) {
        const f3 dir = direct;
        direct = occluded ? mk(0) : pend;  // an occluded light contributes exactly +0 (directIfVisible's rule)
        if (occluded) status |= BDPT_GI_STATUS_DIRECT_OCCLUDED;
        if (indirect) {
          phase = 1u;
          travInit(T, T.o, dir, Q.range.minT, 1e+38f);  // the lane keeps its slot
          retire = false;
        } else {
          giStoreNoHit(Q, rid);
        }
      } else if (phase == 1u) {
        // IndirectMiss (.hlsl:61-73): the environment toward the bounce direction
        bounce = Q.envMap ? envLookup(Q.envMap, Q.envW, Q.envH, T.d) : ld3(Q.envColor);
        giStoreHit(Q, rid, T.best);
      } else {
        bounce = occluded ? mk(0) : pend;
        if (occluded) status |= BDPT_GI_STATUS_BOUNCE_OCCLUDED;
      }
      if (retire) {
#if BDPT_GI_RELOAD_DIFFUSE
        const f3 dif = indirect ? itemDiffuse<SRC>(Q, rid) : mk(0);
#else
        const f3 dif = keptDif;
#endif
        giRetire<SRC>(Q, rid, indirect, direct, bounce, NdotL, dif, status, seed);
        has = false;
        T.cur = kDone;
      }
    }
    // the lanes whose bounce ray hit, together (parkedDue)
    if (parkedDue<BDPT_GI_SHADE_MIN>(parked, has && !parked) && parked) {
      // IndirectClosestHit (.hlsl:85-108): the hit as bdpt_shade_hits shades it, then its NEE term on a copy of the state
      parked = false;
      giStoreHit(Q, rid, T.best);
      status |= BDPT_GI_STATUS_BOUNCE_HIT;
      const f3 from = (Q.flags & BDPT_GI_SHADE_FROM_VIEW) ? ld3(Q.viewPos) : T.o;
      const Shading sd = shadeHit<NMAP>(S, (uint32_t)T.best.prim, T.best.u, T.best.v, from);
      uint32_t t = seed;
      f3 L;
      float dist;
      pend = giNee(S, t, sd.posW, sd.N, sd.diffuse, L, dist);
      giShadowRay(T, pend, sd.posW, L, Q.range.minT, dist);
      phase = 2u;
    }
  }
  releaseCursor(cursor, lane);
}

void launchGi(const SceneDev& S, const GiDev& Q, bool gbuffer, bool normalMap, unsigned long long* cursor, LaunchGrids& G, int numCUs,
              hipStream_t st) {
  if (!Q.range.cap) return;
  if (gbuffer) {  // the pass: full prepareShadingData, so always with the normal map
    launchPersistent(gi_kernel<ITEM_SRC_GBUFFER, true>, G.gi[2], Q.range.cap, numCUs, st, S, Q, cursor);
    return;
  }
  withFlag(normalMap, [&](auto NMAP) {
    launchPersistent(gi_kernel<ITEM_SRC_SURFACES, NMAP>, G.gi[NMAP ? 1 : 0], Q.range.cap, numCUs, st, S, Q, cursor);
  });
}

}  // namespace bdpt
