// deform.hip — the deformation pass of bdpt_update_skinned and bdpt_update_morphed: every vertex morphed (blend-shape
// deltas scaled by the frame's weights and added to the base pose) and / or skinned (blended from up to four bone
// matrices) into the context's output streams, which the refit (refit.hip) then consumes.  What SkinningCache::update
// dispatches in the reference (ComputeSkinning.cs.slang) before RtScene refits its acceleration structure.  Morph and
// skin happen in the same registers: there is no intermediate stream between them.
//
// One lane per vertex on a dense grid of one-wave workgroups; the per-vertex arithmetic is morphVertex of morph.h and
// skinVertex of skin.h, the functions bdpt_host_morph and bdpt_host_skin run on the CPU.  One template, three passes:
//   SKIN          skinning alone.  Bandwidth-bound (60 B read, 36 B written per vertex); the only irregular access is the
//                 palette gather, 112 B per bone.
//   MORPH, SKIN   every vertex: morph, skinVertex, the skin's own streams are written.  A lane reads its entry range from
//                 the vertex-major `start` array (8 B per vertex on top of the above), then per entry the target id and
//                 that target's weight (four entries at a time), and the entry's deltas only when the weight is not
//                 zero.  Weights (at most 4 KB) are gathered from global memory, where they stay in the caches.
//   MORPH         only the vertices that own entries (MorphDev::active), into the morph's own streams: all others hold
//                 the base from bdpt_set_morph on.
// Skinning alone is its own instance, not a morph without entries: it neither takes nor reads the morph (DESIGN.md
// "Morph targets" has what the zero-weight morph costs).  With a skin the palette gather has two paths (DESIGN.md
// "Skinning"):
//   global   the gather goes to global memory (the palette, a few KB, stays in the caches);
//   LDS      palettes of at most kSkinLdsBones bones on skins of at least kSkinLdsMinVertices vertices: each workgroup
//            copies both palettes into LDS once and deforms kDeformLdsChunks consecutive chunks of 64 vertices from there.
#include "morph.h"

#include "kernels.h"

#include "device_trace.hpp"  // BDPT_ONE_WAVE_PER_GROUP
#include "launch.hpp"

namespace bdpt {

constexpr uint32_t kDeformLdsChunks = 16;  // chunks of 64 vertices per workgroup of the LDS path

// what a kernel takes of the morph: nothing at all without MORPH
template <bool MORPH>
struct MorphIn {};
template <>
struct MorphIn<true> {
  MorphDev M;
  const float* weights;
};

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

// Vertex i.  SKIN: the context has a skin K, and N, B say whether it has normals / bitangents (a morph's dNrm / dBit may
// be null all the same); `bones` / `nbones`: the palettes (global or LDS).  !SKIN: N, B say whether the morph has normal /
// bitangent deltas (a base stream without deltas never changes: it is not visited), and K is not read.
template <bool MORPH, bool SKIN, bool N, bool B>
__device__ __forceinline__ void deformOne(const MorphIn<MORPH>& in, const SkinDev& K, const float* bones, const float* nbones, uint32_t i) {
  static_assert(MORPH || SKIN, "nothing to do");
  const size_t o = (size_t)i * 3;
  float p[3], n[3] = {0.0f, 0.0f, 0.0f}, b[3] = {0.0f, 0.0f, 0.0f};
  if constexpr (SKIN) {
    load3(K.restPos, o, p);
    if (N) load3(K.restNrm, o, n);
    if (B) load3(K.restBit, o, b);
  } else {
    load3(in.M.basePos, o, p);
    if (N) load3(in.M.baseNrm, o, n);
    if (B) load3(in.M.baseBit, o, b);
  }
  if constexpr (MORPH) {
    const MorphDev& M = in.M;
    morphVertex(M.target, M.dPos, N ? M.dNrm : nullptr, B ? M.dBit : nullptr, in.weights, M.start[i], M.start[i + 1], p, n, b);
  }
  if constexpr (SKIN) {
    const float4 w4 = reinterpret_cast<const float4*>(K.weights)[i];
    const float w[4] = {w4.x, w4.y, w4.z, w4.w};
    float op[3] = {p[0], p[1], p[2]}, on[3] = {n[0], n[1], n[2]}, ob[3] = {b[0], b[1], b[2]};
    if (!skinIsStatic(w)) {  // (a static vertex: its rest or morphed values, its ids are not read)
      const uint2 id2 = reinterpret_cast<const uint2*>(K.ids)[i];
      const uint16_t id[4] = {(uint16_t)(id2.x & 0xffffu), (uint16_t)(id2.x >> 16), (uint16_t)(id2.y & 0xffffu), (uint16_t)(id2.y >> 16)};
      skinVertex<N, B>(bones, nbones, id, w, p, n, b, op, on, ob);
    }
    store3(K.pos, o, op);
    if (N) store3(K.nrm, o, on);
    if (B) store3(K.bit, o, ob);
  } else {
    store3(in.M.pos, o, p);
    if (N) store3(in.M.nrm, o, n);
    if (B) store3(in.M.bit, o, b);
  }
}

template <bool MORPH, bool SKIN, bool N, bool B>
__global__ __launch_bounds__(kWave) void deform_kernel(SkinDev K, const float* __restrict__ bones, const float* __restrict__ nbones, MorphIn<MORPH> in) {
  BDPT_ONE_WAVE_PER_GROUP();
  const uint32_t j = blockIdx.x * kWave + threadIdx.x;
  if constexpr (SKIN) {
    if (j >= K.numVertices) return;
    deformOne<MORPH, true, N, B>(in, K, bones, nbones, j);
  } else {
    if (j >= in.M.numActive) return;
    deformOne<MORPH, false, N, B>(in, K, bones, nbones, in.M.active[j]);
  }
}

// the palettes staged in LDS once per workgroup, which deforms kDeformLdsChunks consecutive chunks of 64 vertices
template <bool MORPH, bool N, bool B>
__global__ __launch_bounds__(kWave) void deform_lds_kernel(SkinDev K, const float* __restrict__ bones, const float* __restrict__ nbones,
                                                           MorphIn<MORPH> in) {
  BDPT_ONE_WAVE_PER_GROUP();
  __shared__ float sB[kSkinLdsBones * 16];
  __shared__ float sT[N ? kSkinLdsBones * 16 : 1];
  const uint32_t nf = (K.numBones < kSkinLdsBones ? K.numBones : kSkinLdsBones) * 16;  // (the launcher keeps numBones <= kSkinLdsBones)
  for (uint32_t k = threadIdx.x; k < nf; k += kWave) {  // (dword copies: a caller's palette need only be 4-byte aligned)
    sB[k] = bones[k];
    if (N) sT[k] = nbones[k];
  }
  __syncthreads();
  const uint32_t first = blockIdx.x * (kDeformLdsChunks * kWave) + threadIdx.x;
  for (uint32_t c = 0; c < kDeformLdsChunks; c++) {
    const uint32_t i = first + c * kWave;
    if (i >= K.numVertices) return;
    deformOne<MORPH, true, N, B>(in, K, sB, sT, i);
  }
}

void launchDeform(const MorphDev* M, const float* weights, const SkinDev* K, const float* bones, const float* normalBones, int path,
                  hipStream_t st) {
  const uint32_t waves = wavesFor(K ? K->numVertices : M ? M->numActive : 0u);
  if (!waves) return;
  const bool lds = K && K->numBones <= kSkinLdsBones && (path == kSkinPathLds || (path == kSkinPathAuto && K->numVertices >= kSkinLdsMinVertices));
  const bool n = K ? K->nrm != nullptr : M->dNrm != nullptr, b = K ? K->bit != nullptr : M->dBit != nullptr;
  withFlag(M != nullptr, [&](auto MORPH) {
    withFlag(n, [&](auto N) {
      withFlag(b, [&](auto B) {
        MorphIn<MORPH> in;
        if constexpr (MORPH) {
          in = {*M, weights};
          if (!K) return launchWave(deform_kernel<true, false, N, B>, waves, st, SkinDev{}, (const float*)nullptr, (const float*)nullptr, in);
        }
        if (lds)
          launchWave(deform_lds_kernel<MORPH, N, B>, (waves + kDeformLdsChunks - 1) / kDeformLdsChunks, st, *K, bones, normalBones, in);
        else
          launchWave(deform_kernel<MORPH, true, N, B>, waves, st, *K, bones, normalBones, in);
      });
    });
  });
}

}  // namespace bdpt
