// area_lights.hip — the emitter table of BDPT_PARAM_AREA_LIGHTS (contract: include/bdpt.h "Area lights"; sampling:
// device_area.hpp).  Everything is made on the device from the shading records and the material table; the host keeps
// no copy of the triangles.
//   build (once per scene):  [mark referenced triangles] -> count per wave -> scan -> compact (ascending primitive order)
//   refresh (build and every bdpt_update_geometry): weights + per-wave scan -> scan of the wave sums -> add
// Every sum has a fixed order (wave scans by shuffles, the wave sums by one wave in order), so a table has the same bits
// on every run.  The kernels are one-wave workgroups launched through launchWave.
#include <hip/hip_runtime.h>

#include "bvh.h"
#include "device_area.hpp"
#include "device_math.hpp"
#include "device_trace.hpp"
#include "kernels.h"
#include "launch.hpp"

namespace bdpt {

#define BD __device__ __forceinline__

namespace {

// emitter: emissive channel constant with a positive luminance, or textured; `textured` says which
BD bool isEmitter(const SceneDev& S, uint32_t t, bool& textured) {
  const uint32_t mid = __float_as_uint(S.shade[(size_t)t * kShadeRecF4 + 6].x);
  const bdpt_material& m = S.materials[mid];
  const uint32_t type = BDPT_FLAG_EMISSIVE_TYPE(m.flags);
  textured = type == BDPT_CHANNEL_TEXTURE;
  return textured || (type == BDPT_CHANNEL_CONST && luminance(ld3(m.emissive)) > 0.0f);
}

BD float waveScanF(float v) {  // inclusive, Hillis-Steele order
  const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const float u = __shfl_up(v, o);
    if (lane >= o) v = v + u;
  }
  return v;
}
BD uint32_t waveScanU(uint32_t v) {
  const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)v, o);
    if (lane >= o) v = v + u;
  }
  return v;
}

// leaves of the refit plan: every triangle record they hold names a referenced input triangle
__global__ __launch_bounds__(kWave) void area_mark_kernel(const BvhRefitNode* __restrict__ nodes, uint32_t numNodes,
                                                          const uint4* __restrict__ recs, uint8_t* __restrict__ referenced) {
  BDPT_ONE_WAVE_PER_GROUP();
  const uint32_t i = blockIdx.x * kWave + threadIdx.x;
  if (i >= numNodes) return;
  const BvhRefitNode nd = nodes[i];
  const uint4* r = recs + (size_t)nd.rec * kRecF4;
  const uint32_t base = r[2].z, offs = r[2].w;  // words 10, 11: childBase, child offsets
  for (uint32_t k = 0; k < nd.nk && k < 4; k++) {
    if (!(nd.kid[k] & kRefitLeaf)) continue;
    const uint32_t at = base + ((offs >> (8 * k)) & 0xffu);
    for (uint32_t j = 0; j < (nd.kid[k] & ~kRefitLeaf); j++) referenced[recs[(size_t)(at + j) * kRecF4].w] = 1;  // word 3: prim
  }
}

__global__ __launch_bounds__(kWave) void area_count_kernel(SceneDev S, uint32_t numTris, const uint8_t* __restrict__ referenced,
                                                           uint32_t* __restrict__ blockCount, uint32_t* __restrict__ counts) {
  BDPT_ONE_WAVE_PER_GROUP();
  const uint32_t t = blockIdx.x * kWave + threadIdx.x;
  bool tex = false;
  const bool e = t < numTris && (!referenced || referenced[t]) && isEmitter(S, t, tex);
  const unsigned long long m = __ballot(e), mt = __ballot(e && tex);
  if (threadIdx.x == 0) {
    blockCount[blockIdx.x] = (uint32_t)__popcll(m);
    atomicAdd(&counts[0], (uint32_t)__popcll(m));  // (integer sums: the same whatever the order)
    atomicAdd(&counts[1], (uint32_t)__popcll(mt));
  }
}

// one wave: exclusive prefix sums of the per-wave emitter counts, in order
__global__ __launch_bounds__(kWave) void area_count_scan_kernel(const uint32_t* __restrict__ blockCount, uint32_t numBlocks,
                                                                uint32_t* __restrict__ blockBase) {
  BDPT_ONE_WAVE_PER_GROUP();
  uint32_t carry = 0;
  for (uint32_t j0 = 0; j0 < numBlocks; j0 += kWave) {
    const uint32_t j = j0 + threadIdx.x;
    const uint32_t v = j < numBlocks ? blockCount[j] : 0u;
    const uint32_t incl = waveScanU(v);
    if (j < numBlocks) blockBase[j] = carry + incl - v;
    carry += (uint32_t)__shfl((int)incl, kWave - 1);
  }
}

// A triangle's alpha-test record: its place in the ascending list of non-opaque triangles (api_scene.cpp alphaTris), kNoAlphaRec
// for an opaque one
BD uint32_t alphaRecOf(const uint32_t* __restrict__ alphaTris, uint32_t numAlphaTris, uint32_t t) {
  uint32_t lo = 0, hi = numAlphaTris;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (alphaTris[mid] < t)
      lo = mid + 1;
    else
      hi = mid;
  }
  return (lo < numAlphaTris && alphaTris[lo] == t) ? lo : kNoAlphaRec;
}

__global__ __launch_bounds__(kWave) void area_compact_kernel(SceneDev S, uint32_t numTris, const uint8_t* __restrict__ referenced,
                                                             const uint32_t* __restrict__ blockBase, const uint32_t* __restrict__ alphaTris,
                                                             uint32_t numAlphaTris, float4* __restrict__ emit) {
  BDPT_ONE_WAVE_PER_GROUP();
  const uint32_t t = blockIdx.x * kWave + threadIdx.x;
  bool tex = false;
  const bool e = t < numTris && (!referenced || referenced[t]) && isEmitter(S, t, tex);
  const unsigned long long m = __ballot(e);
  if (!e) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t at = blockBase[blockIdx.x] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  emit[at] = make_float4(__uint_as_float(t), __uint_as_float(alphaRecOf(alphaTris, numAlphaTris, t)), 0.0f, 0.0f);
}

// weights w = area * lambda from the current shading records, and each wave's inclusive scan of them
__global__ __launch_bounds__(kWave) void area_weights_kernel(SceneDev S, AreaDev A, float* __restrict__ blockSum,
                                                             uint32_t* __restrict__ blockLast) {
  BDPT_ONE_WAVE_PER_GROUP();
  const uint32_t i = blockIdx.x * kWave + threadIdx.x;
  float w = 0.0f;
  if (i < A.n) {
    float4* e = const_cast<float4*>(A.emit) + i;
    const uint32_t t = __float_as_uint(e->x);
    const float4* sr = S.shade + (size_t)t * kShadeRecF4;
    const float4 q0 = sr[0], q2 = sr[2], q4 = sr[4];
    const f3 p0 = mk(q0.x, q0.y, q0.z), p1 = mk(q2.x, q2.y, q2.z), p2 = mk(q4.x, q4.y, q4.z);
    const float area = 0.5f * length(cross(p1 - p0, p2 - p0));
    bool tex = false;
    (void)isEmitter(S, t, tex);
    const bdpt_material& m = S.materials[__float_as_uint(sr[6].x)];
    const float lambda = tex ? 1.0f : luminance(ld3(m.emissive));
    w = area * lambda;
    e->z = w;
    e->w = area;
  }
  const float incl = waveScanF(w);
  if (i < A.n) const_cast<float*>(A.cdf)[i] = incl;
  const unsigned long long pos = __ballot(i < A.n && w > 0.0f);
  if (threadIdx.x == kWave - 1) {
    blockSum[blockIdx.x] = incl;
    blockLast[blockIdx.x] = pos ? blockIdx.x * kWave + (uint32_t)(63 - __clzll((long long)pos)) : 0xFFFFFFFFu;
  }
}

// one wave: the exclusive prefix of the wave sums, in order (in place), and the last emitter with a positive weight
__global__ __launch_bounds__(kWave) void area_weights_scan_kernel(AreaDev A, float* __restrict__ blockSum, const uint32_t* __restrict__ blockLast,
                                                                  uint32_t numBlocks) {
  BDPT_ONE_WAVE_PER_GROUP();
  float carry = 0.0f;
  uint32_t last = 0xFFFFFFFFu;
  for (uint32_t j0 = 0; j0 < numBlocks; j0 += kWave) {
    const uint32_t j = j0 + threadIdx.x;
    const float v = j < numBlocks ? blockSum[j] : 0.0f;
    const float incl = waveScanF(v);
    const float prev = __shfl_up(incl, 1);
    if (j < numBlocks) blockSum[j] = threadIdx.x == 0 ? carry : carry + prev;
    carry = carry + __shfl(incl, kWave - 1);
    const uint32_t bl = j < numBlocks ? blockLast[j] : 0xFFFFFFFFu;
    const unsigned long long has = __ballot(bl != 0xFFFFFFFFu);
    if (has) last = (uint32_t)__shfl((int)bl, 63 - __clzll((long long)has));
  }
  if (threadIdx.x == 0) const_cast<float*>(A.total)[1] = __uint_as_float(last);
}

// cdf = wave prefix + in-wave scan; W = cdf[n - 1]
__global__ __launch_bounds__(kWave) void area_add_kernel(AreaDev A, const float* __restrict__ blockSum) {
  BDPT_ONE_WAVE_PER_GROUP();
  const uint32_t i = blockIdx.x * kWave + threadIdx.x;
  if (i >= A.n) return;
  float* cdf = const_cast<float*>(A.cdf);
  const float v = blockIdx.x == 0 ? cdf[i] : blockSum[blockIdx.x] + cdf[i];
  cdf[i] = v;
  if (i == A.n - 1) const_cast<float*>(A.total)[0] = v;
}

// bdpt_test_area_light_sample: the functions the AREA instances call, on caller states (16 floats per item)
__global__ __launch_bounds__(kWave) void test_area_kernel(SceneDev S, AreaDev A, int mode, const uint32_t* __restrict__ states,
                                                          const float* __restrict__ points, uint32_t n, float* __restrict__ out) {
  BDPT_ONE_WAVE_PER_GROUP();
  const uint32_t i = blockIdx.x * kWave + threadIdx.x;
  if (i >= n) return;
  float o[16];
#pragma unroll
  for (int k = 0; k < 16; k++) o[k] = 0.0f;
  const float W = areaTotal(A);
  if (W > 0.0f) {
    if (mode == 0) {
      uint32_t seed = states[i];
      f3 nrm, dir, col;
      const AreaPoint x = areaLightStart(S, A, W, seed, nrm, dir, col);
      const float v[16] = {__uint_as_float(x.prim), x.b1, x.b2, x.pos.x, x.pos.y, x.pos.z, nrm.x, nrm.y, nrm.z,
                           dir.x, dir.y, dir.z, col.x, col.y, col.z, __uint_as_float(seed)};
#pragma unroll
      for (int k = 0; k < 16; k++) o[k] = v[k];
    } else {
      f3 L, I;
      float d;
      const AreaPoint x = areaNee(S, A, W, states[i], ld3(points + (size_t)i * 3), L, d, I);
      const float v[13] = {__uint_as_float(x.prim), L.x, L.y, L.z, d, I.x, I.y, I.z, x.b1, x.b2, x.pos.x, x.pos.y, x.pos.z};
#pragma unroll
      for (int k = 0; k < 13; k++) o[k] = v[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 16; k++) out[(size_t)i * 16 + k] = o[k];
}

// bdpt_test_alpha: the alpha verdict of (prim, u, v) from the device functions the traversal calls.  variant 0:
// alphaTestFails; 1: alphaTestFails2 with the item in slot 0 and the next item (the first after the last) in slot 1;
// 2: the slots swapped and the partner's `need` off.  An opaque triangle has no record and passes.
__global__ __launch_bounds__(kWave) void test_alpha_kernel(SceneDev S, const uint32_t* __restrict__ alphaTris, uint32_t numAlphaTris,
                                                           uint32_t variant, const uint32_t* __restrict__ prim,
                                                           const float* __restrict__ uv, uint32_t n, uint8_t* __restrict__ out) {
  BDPT_ONE_WAVE_PER_GROUP();
  const uint32_t i = blockIdx.x * kWave + threadIdx.x;
  if (i >= n) return;
  const uint32_t j = (i + 1 == n) ? 0u : i + 1;
  const uint32_t rec = alphaRecOf(alphaTris, numAlphaTris, prim[i]), other = alphaRecOf(alphaTris, numAlphaTris, prim[j]);
  const float u = uv[(size_t)i * 2], v = uv[(size_t)i * 2 + 1], pu = uv[(size_t)j * 2], pv = uv[(size_t)j * 2 + 1];
  bool fails = false, partner = false;
  if (rec != kNoAlphaRec) {
    if (variant == 0)
      fails = alphaTestFails(S, rec, u, v);
    else if (variant == 1)
      alphaTestFails2(S, true, rec, u, v, other != kNoAlphaRec, other, pu, pv, fails, partner);
    else
      alphaTestFails2(S, false, other, pu, pv, true, rec, u, v, partner, fails);
  }
  out[i] = fails ? 1 : 0;
}

}  // namespace

void launchAreaMarkReferenced(const BvhRefitNode* nodes, uint32_t numNodes, const uint4* recs, uint8_t* referenced, hipStream_t st) {
  if (!numNodes) return;
  launchWave(area_mark_kernel, wavesFor(numNodes), st, nodes, numNodes, recs, referenced);
}
void launchAreaCount(const SceneDev& S, uint32_t numTris, const uint8_t* referenced, uint32_t* blockCount, uint32_t* blockBase,
                     uint32_t* counts, hipStream_t st) {
  if (!numTris) return;
  const uint32_t nb = wavesFor(numTris);
  launchWave(area_count_kernel, nb, st, S, numTris, referenced, blockCount, counts);
  launchWave(area_count_scan_kernel, 1u, st, (const uint32_t*)blockCount, nb, blockBase);
}
void launchAreaCompact(const SceneDev& S, uint32_t numTris, const uint8_t* referenced, const uint32_t* blockBase,
                       const uint32_t* alphaTris, uint32_t numAlphaTris, float4* emit, hipStream_t st) {
  if (!numTris) return;
  launchWave(area_compact_kernel, wavesFor(numTris), st, S, numTris, referenced, blockBase, alphaTris, numAlphaTris, emit);
}
void launchAreaRefresh(const SceneDev& S, const AreaDev& A, float* blockSum, uint32_t* blockLast, hipStream_t st) {
  if (!A.n) return;
  const uint32_t nb = wavesFor(A.n);
  launchWave(area_weights_kernel, nb, st, S, A, blockSum, blockLast);
  launchWave(area_weights_scan_kernel, 1u, st, A, blockSum, (const uint32_t*)blockLast, nb);
  launchWave(area_add_kernel, nb, st, A, (const float*)blockSum);
}
void launchTestAreaSample(const SceneDev& S, const AreaDev& A, int mode, const uint32_t* states, const float* points, uint32_t n,
                          float* out, hipStream_t st) {
  if (!n) return;
  launchWave(test_area_kernel, wavesFor(n), st, S, A, mode, states, points, n, out);
}

void launchTestAlpha(const SceneDev& S, const uint32_t* alphaTris, uint32_t numAlphaTris, uint32_t variant, const uint32_t* prim,
                     const float* uv, uint32_t n, uint8_t* out, hipStream_t st) {
  if (!n) return;
  launchWave(test_alpha_kernel, wavesFor(n), st, S, alphaTris, numAlphaTris, variant, prim, uv, n, out);
}

#undef BD
}  // namespace bdpt
