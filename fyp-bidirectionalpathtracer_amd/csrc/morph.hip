// morph.hip — the morph pass of bdpt_update_morphed: blend-shape deltas scaled by the frame's weights and added to the
// base pose, and, for a context with a skin, the skinning of the result in the same registers; the refit (refit.hip)
// then consumes the streams.  There is no intermediate stream between morph and skin.
//
// One lane per vertex on a dense grid of one-wave workgroups; the per-vertex arithmetic is morphVertex of morph.h and
// skinVertex of skin.h, the functions bdpt_host_morph runs on the CPU.  A lane reads its entry range from the
// vertex-major `start` array (8 B per vertex on top of the skin kernel's 96 B), then per entry the target id and that
// target's weight (four entries at a time), and the entry's deltas only when the weight is not zero.  Weights (at most
// 4 KB) are gathered from global memory, where they stay in the caches.
//   SKIN   every vertex: morph, skinVertex, the skin's own skinned streams are written.  The palette gather has the two
//          paths of skin.hip, chosen by the same rule (DESIGN.md "Morph targets"): global memory, or, for palettes of at
//          most kSkinLdsBones bones on skins of at least kSkinLdsMinVertices vertices, LDS;
//   !SKIN  only the vertices that own entries (MorphDev::active): all others hold the base from bdpt_set_morph on.
#include "morph.h"

#include "kernels.h"

#include "device_trace.hpp"  // BDPT_ONE_WAVE_PER_GROUP
#include "launch.hpp"

namespace bdpt {

__device__ __forceinline__ void load3(const float* s, size_t o, float* v) {
  v[0] = s[o];
  v[1] = s[o + 1];
  v[2] = s[o + 2];
}
__device__ __forceinline__ void store3(float* s, size_t o, const float* v) {
  s[o] = v[0];
  s[o + 1] = v[1];
  s[o + 2] = v[2];
}

constexpr uint32_t kMorphLdsChunks = 16;  // chunks of 64 vertices per workgroup of the LDS path (skin.hip kSkinLdsChunks)

// Vertex i.  SKIN: the context has a skin, and N, B say whether it has normals / bitangents (the morph's dNrm / dBit may
// be null all the same); `bones` / `nbones`: the palettes (global or LDS).  !SKIN: N, B say whether the morph has normal /
// bitangent deltas (a base stream without deltas never changes: it is not visited), and K is not read.
template <bool SKIN, bool N, bool B>
__device__ __forceinline__ void morphOne(const MorphDev& M, const SkinDev& K, const float* weights, const float* bones, const float* nbones,
                                         uint32_t i) {
  const size_t o = (size_t)i * 3;
  const uint32_t e0 = M.start[i], e1 = M.start[i + 1];
  float p[3], n[3] = {0.0f, 0.0f, 0.0f}, b[3] = {0.0f, 0.0f, 0.0f};
  load3(SKIN ? K.restPos : M.basePos, o, p);
  if (N) load3(SKIN ? K.restNrm : M.baseNrm, o, n);
  if (B) load3(SKIN ? K.restBit : M.baseBit, o, b);
  morphVertex(M.target, M.dPos, N ? M.dNrm : nullptr, B ? M.dBit : nullptr, weights, e0, e1, p, n, b);
  if constexpr (SKIN) {
    const float4 w4 = reinterpret_cast<const float4*>(K.weights)[i];
    const float w[4] = {w4.x, w4.y, w4.z, w4.w};
    float op[3] = {p[0], p[1], p[2]}, on[3] = {n[0], n[1], n[2]}, ob[3] = {b[0], b[1], b[2]};
    if (!skinIsStatic(w)) {  // (a static vertex: its morphed values, its ids are not read)
      const uint2 id2 = reinterpret_cast<const uint2*>(K.ids)[i];
      const uint16_t id[4] = {(uint16_t)(id2.x & 0xffffu), (uint16_t)(id2.x >> 16), (uint16_t)(id2.y & 0xffffu), (uint16_t)(id2.y >> 16)};
      skinVertex<N, B>(bones, nbones, id, w, p, n, b, op, on, ob);
    }
    store3(K.pos, o, op);
    if (N) store3(K.nrm, o, on);
    if (B) store3(K.bit, o, ob);
  } else {
    store3(M.pos, o, p);
    if (N) store3(M.nrm, o, n);
    if (B) store3(M.bit, o, b);
  }
}

template <bool SKIN, bool N, bool B>
__global__ __launch_bounds__(kWave) void morph_kernel(MorphDev M, SkinDev K, const float* __restrict__ weights, const float* __restrict__ bones,
                                                      const float* __restrict__ nbones) {
  BDPT_ONE_WAVE_PER_GROUP();
  const uint32_t j = blockIdx.x * kWave + threadIdx.x;
  if (j >= (SKIN ? K.numVertices : M.numActive)) return;
  morphOne<SKIN, N, B>(M, K, weights, bones, nbones, SKIN ? j : M.active[j]);
}

// the palettes staged in LDS once per workgroup, which morphs and skins kMorphLdsChunks consecutive chunks of 64 vertices
template <bool N, bool B>
__global__ __launch_bounds__(kWave) void morph_lds_kernel(MorphDev M, SkinDev K, const float* __restrict__ weights, const float* __restrict__ bones,
                                                          const float* __restrict__ nbones) {
  BDPT_ONE_WAVE_PER_GROUP();
  __shared__ float sB[kSkinLdsBones * 16];
  __shared__ float sT[N ? kSkinLdsBones * 16 : 1];
  const uint32_t nf = (K.numBones < kSkinLdsBones ? K.numBones : kSkinLdsBones) * 16;  // (the launcher keeps numBones <= kSkinLdsBones)
  for (uint32_t k = threadIdx.x; k < nf; k += kWave) {  // (dword copies: a caller's palette need only be 4-byte aligned)
    sB[k] = bones[k];
    if (N) sT[k] = nbones[k];
  }
  __syncthreads();
  const uint32_t first = blockIdx.x * (kMorphLdsChunks * kWave) + threadIdx.x;
  for (uint32_t c = 0; c < kMorphLdsChunks; c++) {
    const uint32_t i = first + c * kWave;
    if (i >= K.numVertices) return;
    morphOne<true, N, B>(M, K, weights, sB, sT, i);
  }
}

template <bool N, bool B>
static void launchMorphT(const MorphDev& M, const SkinDev* K, bool lds, const float* weights, const float* bones, const float* nbones,
                         hipStream_t st) {
  if (!K)
    launchWave(morph_kernel<false, N, B>, wavesFor(M.numActive), st, M, SkinDev{}, weights, bones, nbones);
  else if (lds)
    launchWave(morph_lds_kernel<N, B>, (wavesFor(K->numVertices) + kMorphLdsChunks - 1) / kMorphLdsChunks, st, M, *K, weights, bones, nbones);
  else
    launchWave(morph_kernel<true, N, B>, wavesFor(K->numVertices), st, M, *K, weights, bones, nbones);
}

void launchMorph(const MorphDev& M, const SkinDev* K, const float* weights, const float* bones, const float* normalBones, int path,
                 hipStream_t st) {
  if (K ? !K->numVertices : !M.numActive) return;
  const bool lds = K && K->numBones <= kSkinLdsBones && (path == kSkinPathLds || (path == kSkinPathAuto && K->numVertices >= kSkinLdsMinVertices));
  const bool n = K ? K->nrm != nullptr : M.dNrm != nullptr, b = K ? K->bit != nullptr : M.dBit != nullptr;
  if (!K) bones = normalBones = nullptr;
  if (n && b)
    launchMorphT<true, true>(M, K, lds, weights, bones, normalBones, st);
  else if (n)
    launchMorphT<true, false>(M, K, lds, weights, bones, normalBones, st);
  else if (b)
    launchMorphT<false, true>(M, K, lds, weights, bones, normalBones, st);
  else
    launchMorphT<false, false>(M, K, lds, weights, bones, normalBones, st);
}

}  // namespace bdpt
