// ao.hip — bdpt_ao_query and bdpt_ao_execute: ambient occlusion, S cosine-weighted any-hit rays per item inside a radius,
// from one persistent kernel.
//
// Replaces the reference's AO pass (CommonPasses/Data/CommonPasses/aoTracing.rt.hlsl:74-122 — the ray generation shader
// with its any-hit / miss pair, lines 50-64 — driven by CommonPasses/AmbientOcclusionPass.cpp:76-96), and the
// loop a caller otherwise runs per sample: bdpt_bsdf_query(SAMPLE, Lambertian) -> glue that builds the rays ->
// bdpt_trace_rays(BDPT_TRACE_ANY) -> a count add.
//
// The loop is the item loop of device_item_loop.hpp (refill, nodePhase, leafPhase, parkedDue), kept here as the kernel's
// own text with any-hit rays: through the helpers the kernel computes the same but compiles to other code, which
// measured slower (DESIGN.md "The shared item loop"); with this text its device code is what it was before the helpers
// existed.  A change to the fetch or to the leaf schedule is made there and here.  Cursor release and launch are shared.
// What is its own is what an answered lane does: a lane owns its item for all S rays.  When its ray is answered it adds
// to its count, draws the next direction (getCosHemisphereSample, the Lambertian sampleBRDF's direction) and starts
// that ray in its own slot; after sample S-1 it retires with one store per output.  No output atomics and no per-ray
// memory traffic: every output word has one writer, whatever the order the lanes run in.  Dead items never take a
// slot: their outputs are written at fetch.  Across the traversal a lane keeps its item, k, count, the RNG state and
// N; the origin lives in the traversal state (TravState::o).  BDPT_AO_RELOAD_N re-reads N from the record at every
// regeneration instead (DESIGN.md "Ambient occlusion" has both resource usages and timings).  The item itself, a record
// or a G-buffer pixel, is read through device_item_source.hpp.
#include "kernels.h"

#include "device_item_loop.hpp"
#include "device_item_source.hpp"
#include "device_math.hpp"
#include "device_query.hpp"
#include "device_scene.hpp"
#include "launch.hpp"

namespace bdpt {

// Lanes whose ray is answered regenerate in place right after the leaf phase (1), or wait ("parked", as
// BDPT_WALKQ_SHADE_MIN of walk_query.hip) until this many of the wave wait or no lane is traversing.  Direction
// generation is a few dozen instructions, unlike walk shading.  Measured with tools/ao_times.py (DESIGN.md "Ambient
// occlusion"), S = 32: 1, 8, 16, 32 waiting lanes give 6.25, 6.30, 6.37, 6.15 ms, all within the spread of two runs of one build.
#ifndef BDPT_AO_GEN_MIN
#define BDPT_AO_GEN_MIN 1
#endif
// 1: N is re-read from the record when a lane regenerates, 0: it stays in three registers across the traversal.
#ifndef BDPT_AO_RELOAD_N
#define BDPT_AO_RELOAD_N 0
#endif

// Waves per SIMD the register allocation aims for (experiment knob, as BDPT_WALKQ_WAVES_PER_EU of walk_query.hip): 5 is
// what the kernel needs without spilling — item, k, count, RNG state and N on top of trace_rays_kernel<2>'s 77 VGPRs; at 6
// (80 VGPRs) the allocator spills 8 to 11 words per lane to scratch (DESIGN.md "Ambient occlusion" has the counts).
#ifndef BDPT_AO_WAVES_PER_EU
#define BDPT_AO_WAVES_PER_EU 5
#endif

namespace {

// the outputs of item `i`: ao = count / S, correctly rounded (aoTracing.rt.hlsl:121)
template <int SRC>
__device__ __forceinline__ void aoStore(const AoDev& A, uint32_t i, uint32_t count, uint32_t seed) {
  const float ao = (float)count / (float)A.samples;
  if (SRC == ITEM_SRC_SURFACES) {
    A.ao[i] = ao;
    if (A.counts) A.counts[i] = count;
    if (A.seedsOut) A.seedsOut[i] = seed;
  } else {
    A.out[A.pix[i]] = make_float4(ao, ao, ao, 1.0f);
  }
}

}  // namespace

// cursor: as releaseCursor has it (both words zero when a launch starts and when it ends).
template <int SRC>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(BDPT_AO_WAVES_PER_EU, 8))) void ao_kernel(
    SceneDev S, AoDev A, unsigned long long* cursor) {
  BDPT_ONE_WAVE_PER_GROUP();
  __shared__ int s_stack[kStackLds * kWave];
  int* stk = s_stack + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  // refill (device_item_loop.hpp), as this kernel's own text: see the head of the file
  const uint32_t n = itemCount(A.range.cap, A.range.count);
  const uint32_t share = (n / gridDim.x + kWave - 1) & ~(uint32_t)(kWave - 1);
  const uint32_t chunk = share < (uint32_t)kWave ? (uint32_t)kWave : (share > kFetchChunk ? kFetchChunk : share);
  bool has = false, exhausted = false, parked = false;
  uint32_t rid = 0, k = 0, count = 0, seed = 0, chunkPos = 0, chunkEnd = 0;
  uint32_t nTris = 0, nAlpha = 0;  // (leafStep's tallies: not kept)
#if !BDPT_AO_RELOAD_N
  f3 keptN = mk(0);
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
          seed = itemSeed<SRC>(A, rid);
          f3 pos = mk(0);
          const f3 N = itemNormal<SRC>(A, rid);
          if (!itemAlive<SRC>(A, rid, pos)) {
            aoStore<SRC>(A, rid, A.samples, seed);  // the background branch: ao = 1, no draw; the lane stays idle
          } else {
            k = 0;
            count = 0;
#if !BDPT_AO_RELOAD_N
            keptN = N;
#endif
            const f3 dir = getCosHemisphereSample(seed, N);
            travInit(T, pos, dir, A.range.minT, A.radius);
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
    // nodePhase<0>, leafPhase<BDPT_TRACE_ANY> and parkedDue<BDPT_AO_GEN_MIN>, as this kernel's own text
#if BDPT_LEAF_WAIT > 0
    {
      uint32_t nNodes = 0;
      int maxSp = 0;
      nodeBurst<0, kStackLds, BDPT_NODE_BURST, false>(S, T, stk, has && !parked, nNodes, maxSp);
    }
    const unsigned long long waitMask = __ballot(has && !parked && T.cur < 0), nodeMask = __ballot(has && !parked && T.cur >= 0);
    const int waitNeed = (__popcll(waitMask | nodeMask) * BDPT_LEAF_WAIT_FRAC8 + 7) >> 3;
    const bool leavesDue = (int)__popcll(waitMask) >= waitNeed || nodeMask == 0ull;
#else
    if (has && !parked)
      while (T.cur >= 0) nodeStep<0, kStackLds>(S, T, stk);
    const bool leavesDue = true;
#endif
    if (leavesDue && has && !parked && T.cur < 0) {
      bool finished = (T.cur == kDone);
      if (!finished) {
        finished = leafStep<BDPT_TRACE_ANY, false>(S, T, nTris, nAlpha);
        if (!finished) {
          T.cur = travPop<kStackLds>(S, T, stk);
          finished = (T.cur == kDone);
        }
      }
      parked = finished;
    }
#if BDPT_AO_GEN_MIN > 1
    const unsigned long long parkedMask = __ballot(parked);
    const bool genPhase = (int)__popcll(parkedMask) >= BDPT_AO_GEN_MIN || (parkedMask != 0ull && __ballot(has && !parked) == 0ull);
#else
    const bool genPhase = true;
#endif
    if (genPhase && parked) {
      parked = false;
      count += (T.best.prim < 0) ? 1u : 0u;  // unoccluded: the payload kept its initial value (aoTracing.rt.hlsl:109-115)
      k++;
      if (k < A.samples) {
#if BDPT_AO_RELOAD_N
        const f3 N = itemNormal<SRC>(A, rid);
#else
        const f3 N = keptN;
#endif
        const f3 dir = getCosHemisphereSample(seed, N);
        travInit(T, T.o, dir, A.range.minT, A.radius);  // the lane keeps its slot
      } else {
        aoStore<SRC>(A, rid, count, seed);
        has = false;
        T.cur = kDone;
      }
    }
  }
  releaseCursor(cursor, lane);
}

void launchAo(const SceneDev& S, const AoDev& A, bool gbuffer, unsigned long long* cursor, LaunchGrids& G, int numCUs, hipStream_t st) {
  if (!A.range.cap) return;
  withFlag(gbuffer, [&](auto GB) {
    launchPersistent(ao_kernel<GB ? ITEM_SRC_GBUFFER : ITEM_SRC_SURFACES>, G.ao[GB ? 1 : 0], A.range.cap, numCUs, st, S, A, cursor);
  });
}

}  // namespace bdpt
