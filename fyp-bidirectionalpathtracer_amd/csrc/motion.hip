// motion.hip — the previous pose of an animated scene (include/bdpt.h "Motion", DESIGN.md "Motion").
//
//   keep_pose_kernel     bdpt_keep_pose: the corner positions of every shading record -> the previous-pose array.  What
//                        Falcor's SkinningCache keeps as gSkinnedPrevPositions (ComputeSkinning.cs.slang), here per
//                        primitive corner instead of per vertex, because the shading records are what every update
//                        path (bdpt_update_geometry, bdpt_update_skinned) ends in.
//   motion_query_kernel  bdpt_motion_query: prevPosAtHit for a caller's bdpt_hit records.
//
// Both stream: one lane per item on a dense grid of one-wave workgroups, a lane past the item count returns.
#include "kernels.h"

#include "device_math.hpp"
#include "device_motion.hpp"
#include "device_query.hpp"
#include "device_trace.hpp"  // BDPT_ONE_WAVE_PER_GROUP
#include "launch.hpp"

namespace bdpt {

// 48 of a record's 128 bytes are read (r0, r2, r4), 48 written; w of the copies is 0
__global__ __launch_bounds__(kWave) void keep_pose_kernel(const float4* __restrict__ shade, uint32_t numTris, float4* __restrict__ prevPose) {
  BDPT_ONE_WAVE_PER_GROUP();
  const uint32_t i = blockIdx.x * kWave + threadIdx.x;
  if (i >= numTris) return;
  const float4* r = shade + (size_t)i * kShadeRecF4;
  const float4 r0 = r[0], r2 = r[2], r4 = r[4];
  float4* o = prevPose + (size_t)i * 3;
  o[0] = make_float4(r0.x, r0.y, r0.z, 0.0f);
  o[1] = make_float4(r2.x, r2.y, r2.z, 0.0f);
  o[2] = make_float4(r4.x, r4.y, r4.z, 0.0f);
}

__global__ __launch_bounds__(kWave) void motion_query_kernel(MotionDev M, uint32_t numTris, const float4* __restrict__ hits, uint32_t cap,
                                                             const uint32_t* count, float4* __restrict__ out) {
  BDPT_ONE_WAVE_PER_GROUP();
  uint32_t i;
  if (queryLanePast(cap, count, i)) return;
  const float4 h = hits[i];
  const int prim = __float_as_int(h.w);
  if (prim < 0 || (uint32_t)prim >= numTris) {
    out[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  const f3 q = prevPosAtHit(M, (uint32_t)prim, h.y, h.z);
  out[i] = make_float4(q.x, q.y, q.z, 1.0f);
}

void launchKeepPose(const float4* shade, uint32_t numTris, float4* prevPose, hipStream_t st) {
  if (!numTris) return;
  launchWave(keep_pose_kernel, wavesFor(numTris), st, shade, numTris, prevPose);
}

void launchMotionQuery(const float4* prevPose, uint32_t numTris, const float4* hits, uint32_t cap, const uint32_t* count, float4* out,
                       hipStream_t st) {
  if (!cap) return;
  MotionDev M{};
  M.prevPose = prevPose;
  launchWave(motion_query_kernel, wavesFor(cap), st, M, numTris, hits, cap, count, out);
}

}  // namespace bdpt
