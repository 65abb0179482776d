// device_motion.hpp — where a hit point was in the previous pose (include/bdpt.h "Motion").
// gbuffer_kernel's MOTION instance (kernels.hip) and motion_query_kernel (motion.hip) both call prevPosAtHit, so the
// G-buffer channel and bdpt_motion_query agree bit for bit.
#pragma once
#include "device_math.hpp"
#include "kernels.h"

namespace bdpt {
#define BD __device__ __forceinline__

// shadeHit's posW (device_scene.hpp) on the previous-pose corners: ((0 + p0*b0) + p1*bu) + p2*bv per component, fp32, no
// contraction (the build's -ffp-contract=off); the leading 0 + decides the sign of a zero, as it does there.
BD f3 prevPosAtHit(const MotionDev& M, uint32_t prim, float bu, float bv) {
  const float4* p = M.prevPose + (size_t)prim * 3;
  const float4 p0 = p[0], p1 = p[1], p2 = p[2];
  const float b0 = 1.0f - bu - bv;
  f3 pos = mk(0);
  pos = pos + mk(p0.x, p0.y, p0.z) * b0;
  pos = pos + mk(p1.x, p1.y, p1.z) * bu;
  pos = pos + mk(p2.x, p2.y, p2.z) * bv;
  return pos;
}

#undef BD
}  // namespace bdpt
