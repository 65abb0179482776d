// refit.h — the device refit of bdpt_update_geometry (refit.hip), as api_deform.cpp drives it.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "bvh.h"

namespace bdpt {

// bdpt_update_geometry (refit.hip): the plan and scratch of a context's refit, all in device memory but levelStart
constexpr uint32_t kRefitPartials = 1024;  // blocks of the scene-box reduction (6 floats of partials each)
struct RefitDev {
  const BvhRefitNode* nodes;
  const uint32_t* levelOrder;
  std::vector<uint32_t> levelStart;  // (host) BvhRefitPlan::levelStart
  float* box;        // 6 per node
  float* childArea;  // 4 per node
  float* partial;    // 6 * kRefitPartials
  float* pad;        // 1
  uint32_t numNodes;
  const float* region;  // kPieceFloats per record (launchRefitRegions): the piece-tight refit; null: the plain one
};
// refits `recs` to `positions` (device, 3 floats per vertex) and rewrites the shading records' positions and, when
// `normals` is given, normals; enqueued on `st`, allocates nothing
void launchRefit(const RefitDev& R, BvhRec* recs, float4* shade, const uint32_t* indices, uint32_t numTris, const float* positions, const float* normals,
                 hipStream_t st);
// bdpt_prepare(BDPT_PREPARE_REFIT_PIECES): the regions (bvh.h "piece-tight refit") of the records AS BUILT into `region`,
// kPieceFloats per record; enqueued on `st`
void launchRefitRegions(const RefitDev& R, const BvhRec* recs, float* region, hipStream_t st);
}  // namespace bdpt
