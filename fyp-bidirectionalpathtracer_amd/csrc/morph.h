// morph.h — morph targets (bdpt_set_morph / bdpt_update_morphed / bdpt_host_morph): the per-vertex arithmetic, shared by
// the device kernels (deform.hip) and the host entry point (api_deform.cpp), the vertex-major layout both read, and the launcher
// of the deformation pass, which api_deform.cpp drives.  The arithmetic is the contract of include/bdpt.h "Morph targets": fp32, no contraction
// (-ffp-contract=off on both sides), one product and one sum per term, terms in ascending target order, a term whose
// weight is zero (either sign) skipped.  Plain C++ apart from the __host__ __device__ markers (texture_planes.h BDPT_HD).
#pragma once
#include <stdint.h>

#include <vector>

#include "skin.h"
#include "texture_planes.h"  // BDPT_HD

namespace bdpt {

// One vertex whose entries are [e0, e1) of the vertex-major arrays: `target` the target of an entry (ascending inside a
// vertex), dPos / dNrm / dBit three floats per entry (dNrm, dBit: null = that stream is not morphed), `weights` one per
// target.  p, n, b come in as the base values and go out morphed: x = x + weights[t] * d for every entry whose weight is
// not zero, so a vertex without such an entry keeps its bits (a -0.0 included).  A delta is read only when its weight
// is not zero.
BDPT_HD void morphVertex(const uint32_t* target, const float* dPos, const float* dNrm, const float* dBit, const float* weights, uint32_t e0,
                         uint32_t e1, float* p, float* n, float* b) {
  // Four entries at a time: their target ids are read together, then their weights, so that a lane waits for two loads
  // per four entries instead of two per entry (the kernel is bound by this chain when few weights are set).  The terms
  // are still added one by one in ascending order; a slot past e1 has weight zero and is skipped like any other.
  for (uint32_t e = e0; e < e1; e += 4) {
    const uint32_t left = e1 - e;
    uint32_t t[4];
    float w[4];
    for (uint32_t k = 0; k < 4; k++) t[k] = k < left ? target[e + k] : 0u;
    for (uint32_t k = 0; k < 4; k++) w[k] = k < left ? weights[t[k]] : 0.0f;
    for (uint32_t k = 0; k < 4; k++) {
      if (w[k] == 0.0f) continue;
      const size_t o = (size_t)(e + k) * 3;
      for (int c = 0; c < 3; c++) p[c] = p[c] + w[k] * dPos[o + c];
      if (dNrm)
        for (int c = 0; c < 3; c++) n[c] = n[c] + w[k] * dNrm[o + c];
      if (dBit)
        for (int c = 0; c < 3; c++) b[c] = b[c] + w[k] * dBit[o + c];
    }
  }
}

// The vertex-major form of a bdpt_morph_desc's target-major entries (a CSR over vertices): vertex v owns entries
// [start[v], start[v + 1]), in ascending target order; `active` lists the vertices that own any, ascending.
struct MorphCsr {
  std::vector<uint32_t> start, target, active;
  std::vector<float> dPos, dNrm, dBit;  // three per entry; dNrm / dBit empty when the desc has none
};
// From arrays that passed the desc checks (targetStart non-decreasing from 0, ids below numVertices and strictly ascending
// inside a target, fewer than 2^31 entries).
inline MorphCsr morphBuildCsr(uint32_t numVertices, uint32_t numTargets, const uint32_t* targetStart, const uint32_t* vertex,
                              const float* dPositions, const float* dNormals, const float* dBitangents) {
  MorphCsr m;
  const size_t ne = targetStart[numTargets];
  m.start.assign((size_t)numVertices + 1, 0);
  for (size_t e = 0; e < ne; e++) m.start[(size_t)vertex[e] + 1]++;
  for (size_t v = 0; v < numVertices; v++) {
    if (m.start[v + 1]) m.active.push_back((uint32_t)v);
    m.start[v + 1] += m.start[v];
  }
  m.target.resize(ne);
  m.dPos.resize(ne * 3);
  if (dNormals) m.dNrm.resize(ne * 3);
  if (dBitangents) m.dBit.resize(ne * 3);
  std::vector<uint32_t> fill(m.start.begin(), m.start.end() - 1);
  for (uint32_t t = 0; t < numTargets; t++)  // (targets in ascending order: so are a vertex's entries)
    for (size_t e = targetStart[t]; e < targetStart[t + 1]; e++) {
      const size_t k = fill[vertex[e]]++;
      m.target[k] = t;
      for (int c = 0; c < 3; c++) {
        m.dPos[k * 3 + c] = dPositions[e * 3 + c];
        if (dNormals) m.dNrm[k * 3 + c] = dNormals[e * 3 + c];
        if (dBitangents) m.dBit[k * 3 + c] = dBitangents[e * 3 + c];
      }
    }
  return m;
}

}  // namespace bdpt

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace bdpt {
// A context's morph, all in device memory (api_deform.cpp bdpt_set_morph).  With a skin the base is the skin's rest pose and the
// outputs are the skin's skinned streams: basePos .. bit are null.  Without one, baseNrm / baseBit and nrm / bit are null
// for a stream the morph lacks, and the outputs hold the base from bdpt_set_morph on.
struct MorphDev {
  const uint32_t* start;   // numVertices + 1
  const uint32_t* target;  // per entry
  const float* dPos;       // per entry x 3
  const float* dNrm;       // null: normals are not morphed
  const float* dBit;
  const uint32_t* active;  // the vertices that own entries, ascending
  const float* basePos;
  const float* baseNrm;
  const float* baseBit;
  float* pos;
  float* nrm;
  float* bit;
  uint32_t numVertices;
  uint32_t numTargets;
  uint32_t numActive;
};
// One deformation pass (deform.hip), enqueued on `st`, allocates nothing.  M: the context's morph or null, with `weights`
// (device, numTargets floats); K: its skin or null, with the palettes `bones` / `normalBones` (device, numBones x 16
// floats; normalBones only read when the skin has normals).  With a skin every vertex is (morphed and) skinned in
// registers into the skin's streams; without one the morph's active vertices are morphed into the morph's own streams.
// `path`: kSkinPath* of skin.h, and without a skin there is nothing to stage.
void launchDeform(const MorphDev* M, const float* weights, const SkinDev* K, const float* bones, const float* normalBones, int path,
                  hipStream_t st);
}  // namespace bdpt
#endif
