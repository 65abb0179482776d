// skin.h — skinning (bdpt_set_skin / bdpt_update_skinned / bdpt_host_skin): the per-vertex arithmetic, shared by the
// device kernels (deform.hip) and the host entry point (api_deform.cpp), and the skin as the kernels see it.
// The arithmetic is the contract of include/bdpt.h "Skinning": fp32, no contraction (-ffp-contract=off on both sides),
// every sum in the order written here.  Plain C++ apart from the __host__ __device__ markers (texture_planes.h BDPT_HD).
#pragma once
#include <stdint.h>

#include "texture_planes.h"  // BDPT_HD

namespace bdpt {

// A vertex whose four weights are all zero (either sign) is static: its outputs are its rest values, its ids are not read.
BDPT_HD bool skinIsStatic(const float* w) { return w[0] == 0.0f && w[1] == 0.0f && w[2] == 0.0f && w[3] == 0.0f; }

// element e of the blended matrix: ((M[i0][e]*w0 + M[i1][e]*w1) + M[i2][e]*w2) + M[i3][e]*w3; m[k] = &M[ik][0]
BDPT_HD float skinBlend(const float* const* m, const float* w, int e) {
  return ((m[0][e] * w[0] + m[1][e] * w[1]) + m[2][e] * w[2]) + m[3][e] * w[3];
}

// One non-static vertex.  `bones` / `normalBones`: the palettes, 16 floats per bone, m[4r+c] (normalBones is read only
// with N).  p, n, b: the rest position, normal, bitangent (n only with N, b only with B); op, on, ob the same for the
// outputs.  Only the twelve elements of the blended matrix that reach an output are formed (columns 0..2), and the nine
// of the blended inverse transpose.
template <bool N, bool B>
BDPT_HD void skinVertex(const float* bones, const float* normalBones, const uint16_t* id, const float* w, const float* p, const float* n,
                        const float* b, float* op, float* on, float* ob) {
  const float* m[4] = {bones + (size_t)id[0] * 16, bones + (size_t)id[1] * 16, bones + (size_t)id[2] * 16, bones + (size_t)id[3] * 16};
  float M[4][3];
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 3; c++) M[r][c] = skinBlend(m, w, 4 * r + c);
  for (int c = 0; c < 3; c++) op[c] = ((p[0] * M[0][c] + p[1] * M[1][c]) + p[2] * M[2][c]) + M[3][c];
  if (B)
    for (int c = 0; c < 3; c++) ob[c] = (b[0] * M[0][c] + b[1] * M[1][c]) + b[2] * M[2][c];
  if (N) {
    const float* t[4] = {normalBones + (size_t)id[0] * 16, normalBones + (size_t)id[1] * 16, normalBones + (size_t)id[2] * 16,
                         normalBones + (size_t)id[3] * 16};
    float T[3][3];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) T[r][c] = skinBlend(t, w, 4 * r + c);
    for (int c = 0; c < 3; c++) on[c] = (n[0] * T[0][c] + n[1] * T[1][c]) + n[2] * T[2][c];
  }
}

}  // namespace bdpt

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace bdpt {
// The LDS path of the kernels (deform.hip, DESIGN.md "Skinning"): palettes of at most kSkinLdsBones bones are staged in LDS
// by each workgroup when the skin has at least kSkinLdsMinVertices vertices (fewer leave the chip short of workgroups:
// measured, the gather from global memory wins below about 0.75 M vertices and loses from about 1.25 M on).  Everything
// else gathers from global memory.
constexpr uint32_t kSkinLdsBones = 64;
constexpr uint32_t kSkinLdsMinVertices = 1u << 20;
// A context's skin, all in device memory (api_deform.cpp bdpt_set_skin).  normals / bitangents (rest and skinned) are null for a
// stream the skin lacks.
struct SkinDev {
  const float* restPos;
  const float* restNrm;
  const float* restBit;
  const float* weights;   // 4 per vertex, 16-byte aligned
  const uint16_t* ids;    // 4 per vertex, 8-byte aligned; below numBones for every non-static vertex
  float* pos;             // the skinned streams, 3 per vertex
  float* nrm;
  float* bit;
  uint32_t numVertices;
  uint32_t numBones;
};
// how launchDeform (morph.h) gathers the palettes: kSkinPathAuto picks by palette size and vertex count; the other two
// force a path (kSkinPathLds falls back to global above kSkinLdsBones)
enum : int { kSkinPathAuto = 0, kSkinPathGlobal = 1, kSkinPathLds = 2 };
}  // namespace bdpt
#endif
