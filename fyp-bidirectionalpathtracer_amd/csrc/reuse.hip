// reuse.hip — bdpt_reuse_query and bdpt_reuse_execute: reservoir reuse, the second stage of ReSTIR behind the resampled
// direct lighting pass (ris.hip).  An item combines its own reservoir with those of up to eight pool entries — spatial
// neighbours, or the same point a frame ago — by the unbiased 1 / Z rule, and one any-hit ray is traced for the
// survivor: the worth of every source's candidates for one re-evaluation each and a single ray.
//
// Replaces the loop a caller otherwise runs per source: prev(state) -> bdpt_light_query(NEE) -> clamp, weight and
// reservoir update, the same again at every neighbour's surface for Z, then bdpt_trace_rays(ANY) (include/bdpt.h
// "Reservoir reuse" has the definition; the two are equal bit for bit).  A sample (light, state) is evaluated by
// lightGiven of device_light.hpp, the text bdpt_light_query itself runs behind its light choice.
//
// Shaped like ris_kernel with one sample per item, on the item loop of device_item_loop.hpp.  A lane owns its item: in
// its ray-less phase it makes all 1 + 2 * neighbors evaluations (every source's sample at the item, then the selected
// sample at every neighbour), then starts its one ray in its own slot, and it retires with one store per output.  Lanes
// with a fresh item wait ("parked") until BDPT_REUSE_REGEN_MIN of the wave do, or none is traversing.  No output atomics:
// every output word has one writer.  Dead items never take a slot: their outputs are written at fetch.
//
// Termination: an item makes its evaluations once and traces at most one ray, and a traversal is finite.  The wave leaves
// when the cursor is exhausted and no lane holds an item.
//
// Across the traversal a lane keeps its item, the term its ray gates, the out record and the RNG state; the origin lives
// in the traversal state.  Nothing a caller supplies reaches an address: a neighbour index is compared with poolNum, a
// light id with the pass's light count, and a count only enters arithmetic.  The item, a record or a G-buffer pixel, is
// read and written through device_item_source.hpp; a pool entry, a record or a pixel of the pool G-buffer, is read here.
#include "kernels.h"

#include "device_item_loop.hpp"
#include "device_item_source.hpp"
#include "device_light.hpp"
#include "device_math.hpp"
#include "device_query.hpp"
#include "device_scene.hpp"
#include "launch.hpp"

namespace bdpt {

// Waves per SIMD the register allocation aims for, chosen as BDPT_RIS_WAVES_PER_EU of ris.hip was: DESIGN.md "Reservoir
// reuse" has the resource usage of the eight instances.
#ifndef BDPT_REUSE_WAVES_PER_EU
#define BDPT_REUSE_WAVES_PER_EU 4
#endif
// ... and of the AREA instances, whose evaluations also hold areaNee's emitter point, and of the GGX G-buffer instance,
// which decodes a pool pixel's half channels and normalises its V beside the item's: at 4 it spilled 20 bytes a lane
#ifndef BDPT_REUSE_WIDE_WAVES_PER_EU
#define BDPT_REUSE_WIDE_WAVES_PER_EU 3
#endif
// Lanes with a fresh item wait until this many of the wave wait, or no lane is traversing, so that the evaluations are
// made for many lanes at once.  1: never wait.  48 is BDPT_RIS_REGEN_MIN of ris.hip carried over; tools/reuse_times.py
// --fused-only compares builds, and the sweep over 1 / 32 / 48 is still to be made (DESIGN.md "Reservoir reuse").
#ifndef BDPT_REUSE_REGEN_MIN
#define BDPT_REUSE_REGEN_MIN 48
#endif

namespace {

constexpr uint32_t kReuseNoLight = BDPT_RIS_NO_LIGHT;
constexpr uint32_t kReuseNone = 0xffffffffu;  // a neighbour slot without a pool entry
constexpr uint32_t kReuseStreamKey = 0x52455553u;  // the execute call's seeds fork from the pixel's with this key

struct ReuseShading {
  f3 N, V, dif, spec;
  float rough;
};

// What a sample's value reads of a surface at `pos`: record `at` of `surf`, or frame pixel `at` of a G-buffer seen from
// `cam`.  The Lambertian instances read N and diffuse only.
template <int SRC, bool GGX>
__device__ __forceinline__ ReuseShading reuseShading(const float4* surf, const uint16_t* gbNormal, const uint16_t* gbDiffuse,
                                                     const uint16_t* gbSpecRough, const float* cam, uint32_t at, f3 pos) {
  ReuseShading sd;
  sd.V = mk(0);
  sd.spec = mk(0);
  sd.rough = 0.0f;
  if (SRC == ITEM_SRC_SURFACES) {
    const float4* r = surf + (size_t)at * 6;
    const float4 q1 = r[1], q3 = r[3];
    sd.N = mk(q1.x, q1.y, q1.z);
    sd.dif = mk(q3.x, q3.y, q3.z);
    if (GGX) {
      const float4 q2 = r[2], q4 = r[4];
      sd.V = mk(q2.x, q2.y, q2.z);
      sd.spec = mk(q4.x, q4.y, q4.z);
      sd.rough = q1.w * q1.w;
    }
  } else {
    sd.N = itemHalf3(gbNormal, at);
    sd.dif = itemHalf3(gbDiffuse, at);
    if (GGX) {  // as risShading of ris.hip reads the pixel
      const uint2 raw = reinterpret_cast<const uint2*>(gbSpecRough)[at];
      sd.spec = mk(f16_to_f32((uint16_t)(raw.x & 0xffffu)), f16_to_f32((uint16_t)(raw.x >> 16)), f16_to_f32((uint16_t)(raw.y & 0xffffu)));
      const float a = f16_to_f32((uint16_t)(raw.y >> 16));
      sd.rough = a * a;
      sd.V = normalize(ld3(cam) - pos);
    }
  }
  return sd;
}

// v_x(y): the clamped value of sample (light, state), light < lightsCount, at the surface (pos, sd); c: its shadow ray
template <bool GGX, bool AREA>
__device__ __forceinline__ f3 reuseValue(const SceneDev& S, const AreaDev& A, float areaW, int lightsCount, uint32_t light, uint32_t state,
                                         f3 pos, const ReuseShading& sd, float clampUpper, LightCandidate& c) {
  return clampVec(lightGiven<GGX, AREA>(S, A, areaW, lightsCount, (int)light, state, pos, sd.N, sd.V, sd.dif, sd.spec, sd.rough, c),
                  clampUpper);
}

// where item `i`'s own record lies in `in` and `res`: at the item, or at its frame pixel
template <int SRC>
__device__ __forceinline__ uint32_t reuseSlot(const ReuseDev& Q, uint32_t i) {
  return SRC == ITEM_SRC_SURFACES ? i : Q.pix[i];
}

// The pool index of neighbour slot n of the item whose records lie at `slot`: the caller's, or for a pixel without a
// caller's image its own pixel (radius 0: slot 0 only) or a pixel at an offset drawn from `so`, which advances twice.
template <int SRC>
__device__ __forceinline__ uint32_t reuseNeighborIndex(const ReuseDev& Q, uint32_t slot, uint32_t n, uint32_t& so) {
  if (SRC == ITEM_SRC_SURFACES || Q.neighborIndex) return Q.neighborIndex[(size_t)slot * Q.neighbors + n];
  if (Q.radius == 0u) return n == 0u ? slot : kReuseNone;
  const float side = (float)(2u * Q.radius + 1u);
  const float u1 = nextRand(so);
  const float u2 = nextRand(so);
  const int dx = (int)(u1 * side) - (int)Q.radius, dy = (int)(u2 * side) - (int)Q.radius;
  const int x = (int)(slot % Q.width) + dx, y = (int)(slot / Q.width) + dy;
  if ((dx == 0 && dy == 0) || x < 0 || y < 0 || x >= (int)Q.width || y >= (int)Q.height) return kReuseNone;
  return (uint32_t)y * Q.width + (uint32_t)x;
}

// Pool entry p as a neighbour of an item at `pos` with normal N: false when the slot is skipped — no such entry, a dead
// one, or one the normal or plane test rejects.
template <int SRC>
__device__ __forceinline__ bool reuseNeighborOk(const ReuseDev& Q, uint32_t p, f3 pos, f3 N) {
  if (p >= Q.poolNum) return false;
  f3 posP, Np;
  if (SRC == ITEM_SRC_SURFACES) {
    if (Q.poolAlive && Q.poolAlive[p] == 0) return false;
    const float4* r = Q.poolSurf + (size_t)p * 6;
    if (__float_as_int(r[5].w) < 0) return false;
    const float4 q0 = r[0], q1 = r[1];
    posP = mk(q0.x, q0.y, q0.z);
    Np = mk(q1.x, q1.y, q1.z);
  } else {
    const float4 wp = Q.poolGbPosition[p];
    if (!(wp.w != 0.0f)) return false;
    posP = mk(wp.x, wp.y, wp.z);
    Np = itemHalf3(Q.poolGbNormal, p);
  }
  if (!(dot(N, Np) >= Q.normalMin)) return false;
  return fabsf(dot(N, posP - pos)) <= Q.planeMax;
}

template <int SRC>
__device__ __forceinline__ f3 reusePoolPos(const ReuseDev& Q, uint32_t p) {
  const float4 q0 = SRC == ITEM_SRC_SURFACES ? Q.poolSurf[(size_t)p * 6] : Q.poolGbPosition[p];
  return mk(q0.x, q0.y, q0.z);
}

// a record's candidate count: the call's scalar when that is set, else the record's M word; at most BDPT_REUSE_MAX_M
__device__ __forceinline__ uint32_t reuseCount(uint32_t scalar, uint32_t word) {
  const uint32_t m = scalar ? scalar : word;
  return m < BDPT_REUSE_MAX_M ? m : BDPT_REUSE_MAX_M;
}
__device__ __forceinline__ uint32_t reusePoolCount(const ReuseDev& Q, uint32_t word) {
  const uint32_t m = reuseCount(Q.poolM, word);
  return m < Q.maxM ? m : Q.maxM;
}

// Item `i` at `pos`: its draws, the selection among the sources and Z.  Returns whether a ray is in flight: then `pend`
// is the term it gates and `rec` the out record (status bit 0 set).  false: nothing was selected, `rec` is the empty
// record with the item's count.
template <int SRC, bool GGX, bool AREA>
__device__ __forceinline__ bool reuseItem(const SceneDev& S, const ReuseDev& Q, const AreaDev& A, uint32_t i, f3 pos, uint32_t& seed, f3& pend,
                                          uint4& rec, TravState& T) {
  const uint32_t slot = reuseSlot<SRC>(Q, i);
  const ReuseShading sd = reuseShading<SRC, GGX>(Q.surf, Q.gbNormal, Q.gbDiffuse, Q.gbSpecRough, Q.camPos, slot, pos);
  float areaW;
  const int lightsCount = lightsCountOf<AREA>(S, A, areaW);
  // drawn offsets come before the selection draws: `seed` skips them, the slots take them from the state before
  const bool drawn = SRC == ITEM_SRC_GBUFFER && !Q.neighborIndex && Q.radius != 0u;
  const uint32_t offsets = seed;
  if (drawn)
    for (uint32_t n = 0; n < 2u * Q.neighbors; n++) nextRand(seed);
  float wsum = 0.0f, tSel = 0.0f;
  uint32_t mTot = 0, used = 0;  // used: bit n = neighbour slot n was not skipped
  f3 vSel = mk(0);
  LightCandidate sel;
  sel.light = -1;
  sel.area = false;
  sel.L = mk(0);
  sel.dist = 0.0f;
  uint32_t stateSel = 0;
  const uint4 own = Q.in[slot];
  const uint32_t mOwn = reuseCount(Q.inM, own.w);
  uint32_t so = offsets;
  for (uint32_t j = 0; j <= Q.neighbors; j++) {
    const float u = nextRand(seed);
    uint4 y = own;
    uint32_t m = mOwn;
    if (j) {
      const uint32_t p = reuseNeighborIndex<SRC>(Q, slot, j - 1u, so);
      if (!reuseNeighborOk<SRC>(Q, p, pos, sd.N)) continue;
      used |= 1u << (j - 1u);
      y = Q.pool[p];
      m = reusePoolCount(Q, y.w);
    }
    mTot += m;
    const uint32_t light = y.x & 0xffffu;  // (BDPT_RIS_NO_LIGHT is no light of any scene: it fails the comparison too)
    const float Wy = __uint_as_float(y.z);
    if (!(light < (uint32_t)lightsCount && Wy > 0.0f)) continue;  // an empty record: w = 0
    LightCandidate cand;
    const f3 v = reuseValue<GGX, AREA>(S, A, areaW, lightsCount, light, y.y, pos, sd, Q.clampUpper, cand);
    const float t = maxf(maxf(v.x, v.y), v.z);
    const float w = (t * Wy) * (float)m;
    wsum = wsum + w;
    if (w > 0.0f && u * wsum <= w) {
      vSel = v;
      tSel = t;
      sel = cand;
      stateSel = y.y;
    }
  }
  rec = make_uint4(kReuseNoLight, 0u, 0u, mTot);
  if (sel.light < 0) return false;
  // Z: the counts of the sources at whose own surface the selected sample has a positive target; the item's own is one of
  // them (a selection's w > 0 needs t > 0 at the item)
  uint32_t Z = mOwn;
  so = offsets;
  for (uint32_t n = 0; n < Q.neighbors; n++) {
    const uint32_t p = reuseNeighborIndex<SRC>(Q, slot, n, so);
    if (!((used >> n) & 1u)) continue;
    const f3 posP = reusePoolPos<SRC>(Q, p);
    const ReuseShading sp = reuseShading<SRC, GGX>(Q.poolSurf, Q.poolGbNormal, Q.poolGbDiffuse, Q.poolGbSpecRough, Q.poolCamPos, p, posP);
    LightCandidate unused;
    const f3 v = reuseValue<GGX, AREA>(S, A, areaW, lightsCount, (uint32_t)sel.light, stateSel, posP, sp, Q.clampUpper, unused);
    if (maxf(maxf(v.x, v.y), v.z) > 0.0f) Z += reusePoolCount(Q, Q.pool[p].w);
  }
  if (Z == 0u) return false;
  const float W = (wsum / (float)Z) / tSel;
  pend = vSel * W;
  rec = make_uint4((uint32_t)sel.light | (BDPT_RIS_STATUS_RAY << 16), stateSel, __float_as_uint(W), mTot);
  travInit(T, pos, sel.L, Q.range.minT, sel.dist);  // the lane keeps its slot
  return true;
}

// every output of item `i`
template <int SRC>
__device__ __forceinline__ void reuseStore(const ReuseDev& Q, uint32_t i, f3 color, uint32_t traced, uint32_t seed, uint4 rec) {
  itemStoreColor<SRC>(Q, i, color);
  if (SRC == ITEM_SRC_SURFACES) {
    if (Q.traced) Q.traced[i] = traced;
    if (Q.seedsOut) Q.seedsOut[i] = seed;
  }
  if (Q.res) Q.res[reuseSlot<SRC>(Q, i)] = rec;
}

}  // namespace

// cursor: as releaseCursor has it (both words zero when a launch starts and when it ends).
template <int SRC, bool GGX, bool AREA>
__global__ __launch_bounds__(kWave)
    __attribute__((amdgpu_waves_per_eu((AREA || (GGX && SRC == ITEM_SRC_GBUFFER)) ? BDPT_REUSE_WIDE_WAVES_PER_EU : BDPT_REUSE_WAVES_PER_EU, 8))) void reuse_kernel(
    SceneDev S, ReuseDev Q, AreaDev A, unsigned long long* cursor) {
  BDPT_ONE_WAVE_PER_GROUP();
  __shared__ int s_stack[kStackLds * kWave];
  int* stk = s_stack + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  ItemFeed F = feedInit(itemCount(Q.range.cap, Q.range.count));
  bool has = false, flying = false;  // flying: the lane's ray is in flight
  uint32_t rid = 0, seed = 0;
  f3 pend = mk(0);
  uint4 rec = make_uint4(0u, 0u, 0u, 0u);
  TravState T;
  T.cur = kDone;
  T.o = mk(0);
  T.best.prim = -1;
  while (refill(F, cursor, lane, has, [&](uint32_t item) {
    f3 pos = mk(0);
    if (!itemAlive<SRC>(Q, item, pos)) {
      // the background: the diffuse channel holds the colour, no draw, the empty record; the lane stays idle.  Only a
      // record's state is stored (unchanged); a pixel's initRand is not made for nothing.
      reuseStore<SRC>(Q, item, itemDiffuse<SRC>(Q, item), 0u, SRC == ITEM_SRC_SURFACES ? itemSeed<SRC>(Q, item) : 0u,
                      make_uint4(kReuseNoLight, 0u, 0u, 0u));
      return;
    }
    rid = item;
    seed = itemSeed<SRC>(Q, item);
    if (SRC == ITEM_SRC_GBUFFER) seed = initRand(seed, kReuseStreamKey);
    T.o = pos;  // the origin of the item's ray
    flying = false;
    has = true;
  })) {
    const bool leavesDue = nodePhase<0>(S, T, stk, flying);
    if (leavesDue && flying && T.cur < 0 && leafPhase<BDPT_TRACE_ANY>(S, T, stk)) {
      const bool occluded = T.best.prim >= 0;
      if (occluded) rec.x |= BDPT_RIS_STATUS_OCCLUDED << 16;
      reuseStore<SRC>(Q, rid, occluded ? mk(0) : pend, 1u, seed, rec);
      flying = false;
      has = false;
      T.cur = kDone;
    }
    if (parkedDue<BDPT_REUSE_REGEN_MIN>(has && !flying, flying) && has && !flying) {
      if (reuseItem<SRC, GGX, AREA>(S, Q, A, rid, T.o, seed, pend, rec, T)) {
        flying = true;
      } else {
        reuseStore<SRC>(Q, rid, mk(0), 0u, seed, rec);
        has = false;
        T.cur = kDone;
      }
    }
  }
  releaseCursor(cursor, lane);
}

void launchReuse(const SceneDev& S, const ReuseDev& Q, const AreaDev& A, bool gbuffer, bool ggx, unsigned long long* cursor, LaunchGrids& G,
                 int numCUs, hipStream_t st) {
  if (!Q.range.cap) return;
  withFlag(gbuffer, [&](auto GB) {
    withFlag(ggx, [&](auto GGX) {
      withFlag(A.n != 0, [&](auto AREA) {
        launchPersistent(reuse_kernel<GB ? ITEM_SRC_GBUFFER : ITEM_SRC_SURFACES, GGX, AREA>, G.reuse[(GB ? 4 : 0) + (GGX ? 2 : 0) + (AREA ? 1 : 0)],
                         Q.range.cap, numCUs, st, S, Q, A, cursor);
      });
    });
  });
}

}  // namespace bdpt
