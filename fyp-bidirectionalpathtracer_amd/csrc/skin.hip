// skin.hip — the skinning pass of bdpt_update_skinned: every vertex blended from up to four bone matrices into the
// context's skinned streams, which the refit (refit.hip) then consumes.  What SkinningCache::update dispatches in the
// reference (ComputeSkinning.cs.slang) before RtScene refits its acceleration structure.
//
// One lane per vertex on a dense grid of one-wave workgroups; the per-vertex arithmetic is skinVertex of skin.h, the
// function bdpt_host_skin runs on the CPU.  The pass is bandwidth-bound (60 B read, 36 B written per vertex); the only
// irregular access is the palette gather, 112 B per bone.  Two paths (DESIGN.md "Skinning"):
//   global   the gather goes to global memory (the palette, a few KB, stays in the caches);
//   LDS      palettes of at most kSkinLdsBones bones on skins of at least kSkinLdsMinVertices vertices: each workgroup
//            copies both palettes into LDS once and skins kSkinLdsChunks consecutive chunks of 64 vertices from there.
#include "skin.h"

#include "kernels.h"

#include "device_trace.hpp"  // BDPT_ONE_WAVE_PER_GROUP
#include "launch.hpp"

namespace bdpt {

constexpr uint32_t kSkinLdsChunks = 16;  // chunks of 64 vertices per workgroup of the LDS path

// vertex i of the skin from the palettes `bones` / `nbones` (global or LDS)
template <bool N, bool B>
__device__ __forceinline__ void skinOne(const SkinDev& K, const float* bones, const float* nbones, uint32_t i) {
  const size_t o = (size_t)i * 3;
  const float4 w4 = reinterpret_cast<const float4*>(K.weights)[i];
  const float w[4] = {w4.x, w4.y, w4.z, w4.w};
  const float p[3] = {K.restPos[o], K.restPos[o + 1], K.restPos[o + 2]};
  float n[3] = {0.0f, 0.0f, 0.0f}, b[3] = {0.0f, 0.0f, 0.0f};
  if (N) {
    n[0] = K.restNrm[o];
    n[1] = K.restNrm[o + 1];
    n[2] = K.restNrm[o + 2];
  }
  if (B) {
    b[0] = K.restBit[o];
    b[1] = K.restBit[o + 1];
    b[2] = K.restBit[o + 2];
  }
  float op[3] = {p[0], p[1], p[2]}, on[3] = {n[0], n[1], n[2]}, ob[3] = {b[0], b[1], b[2]};
  if (!skinIsStatic(w)) {  // (a static vertex: rest values, its ids are not read)
    const uint2 id2 = reinterpret_cast<const uint2*>(K.ids)[i];
    const uint16_t id[4] = {(uint16_t)(id2.x & 0xffffu), (uint16_t)(id2.x >> 16), (uint16_t)(id2.y & 0xffffu), (uint16_t)(id2.y >> 16)};
    skinVertex<N, B>(bones, nbones, id, w, p, n, b, op, on, ob);
  }
  K.pos[o] = op[0];
  K.pos[o + 1] = op[1];
  K.pos[o + 2] = op[2];
  if (N) {
    K.nrm[o] = on[0];
    K.nrm[o + 1] = on[1];
    K.nrm[o + 2] = on[2];
  }
  if (B) {
    K.bit[o] = ob[0];
    K.bit[o + 1] = ob[1];
    K.bit[o + 2] = ob[2];
  }
}

template <bool N, bool B>
__global__ __launch_bounds__(kWave) void skin_kernel(SkinDev K, const float* __restrict__ bones, const float* __restrict__ nbones) {
  BDPT_ONE_WAVE_PER_GROUP();
  const uint32_t i = blockIdx.x * kWave + threadIdx.x;
  if (i >= K.numVertices) return;
  skinOne<N, B>(K, bones, nbones, i);
}

template <bool N, bool B>
__global__ __launch_bounds__(kWave) void skin_lds_kernel(SkinDev K, const float* __restrict__ bones, const float* __restrict__ nbones) {
  BDPT_ONE_WAVE_PER_GROUP();
  __shared__ float sB[kSkinLdsBones * 16];
  __shared__ float sT[N ? kSkinLdsBones * 16 : 1];
  const uint32_t nf = (K.numBones < kSkinLdsBones ? K.numBones : kSkinLdsBones) * 16;  // (the launcher keeps numBones <= kSkinLdsBones)
  for (uint32_t k = threadIdx.x; k < nf; k += kWave) {  // (dword copies: a caller's palette need only be 4-byte aligned)
    sB[k] = bones[k];
    if (N) sT[k] = nbones[k];
  }
  __syncthreads();
  const uint32_t first = blockIdx.x * (kSkinLdsChunks * kWave) + threadIdx.x;
  for (uint32_t c = 0; c < kSkinLdsChunks; c++) {
    const uint32_t i = first + c * kWave;
    if (i >= K.numVertices) return;
    skinOne<N, B>(K, sB, sT, i);
  }
}

template <bool N, bool B>
static void launchSkinT(const SkinDev& K, const float* bones, const float* nbones, bool lds, hipStream_t st) {
  const uint32_t chunks = wavesFor(K.numVertices);
  if (lds)
    launchWave(skin_lds_kernel<N, B>, (chunks + kSkinLdsChunks - 1) / kSkinLdsChunks, st, K, bones, nbones);
  else
    launchWave(skin_kernel<N, B>, chunks, st, K, bones, nbones);
}

void launchSkin(const SkinDev& K, const float* bones, const float* normalBones, int path, hipStream_t st) {
  if (!K.numVertices) return;
  const bool lds = K.numBones <= kSkinLdsBones && (path == kSkinPathLds || (path == kSkinPathAuto && K.numVertices >= kSkinLdsMinVertices));
  const bool n = K.nrm != nullptr, b = K.bit != nullptr;
  if (n && b)
    launchSkinT<true, true>(K, bones, normalBones, lds, st);
  else if (n)
    launchSkinT<true, false>(K, bones, normalBones, lds, st);
  else if (b)
    launchSkinT<false, true>(K, bones, normalBones, lds, st);
  else
    launchSkinT<false, false>(K, bones, normalBones, lds, st);
}

}  // namespace bdpt
