// refit.hip — bdpt_update_geometry on the device: the acceleration structure bdpt_set_scene built, refitted in place to
// new vertex positions, and the per-triangle shading records rewritten.  Replaces the in-place update of the DXR driver's
// acceleration structure that Falcor requests every frame (RtScene::update marks it for refit, RtScene.cpp:74-83;
// RtScene::createTlas then builds with PERFORM_UPDATE, RtScene.cpp:244-283).
//
// What is rewritten and with which arithmetic is bvh.h "refit" (bvhRefitNode, bvhQuantiseNode, bvhTriGeom): the same
// functions the host refit (bvh_build.cpp bvhRefitHost) runs, so the two give the same records bit for bit.  Order:
//   1. the scene box over every input triangle (block partials, then one block) -> the pad of buildBvh, in device memory
//   2. one launch per level of the plan, deepest first: a thread per node rewrites its leaf children's triangle records,
//      takes the union of its children's exact boxes and quantises (min / max only: no order dependence)
//   3. the shading records (positions, normals when given)
// With regions (bdpt_prepare(BDPT_PREPARE_REFIT_PIECES), made once by k_refit_regions from the tree as built) step 2 runs
// its piece-tight instance: a split or clipped reference is bounded by its piece, not by its whole triangle.
// Nothing here allocates or synchronises: the plan and the scratch are the caller's (api_deform.cpp), so an update with
// device-pointer inputs can be captured into a hipGraph.
#include <hip/hip_runtime.h>

#include "bvh.h"
#include "kernels.h"
#include "refit.h"

namespace bdpt {
namespace {

constexpr uint32_t kBoxBlock = 256;

__global__ __launch_bounds__(kBoxBlock) void k_refit_scene_box(const float* __restrict__ pos, const uint32_t* __restrict__ idx, uint32_t numTris,
                                                              float* __restrict__ partial) {
  __shared__ float s[6][kBoxBlock];
  float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
  for (uint32_t t = blockIdx.x * kBoxBlock + threadIdx.x; t < numTris; t += gridDim.x * kBoxBlock) {
    float v0[3], e1[3], e2[3], tl[3], th[3];
    bvhTriGeom(pos + (size_t)idx[(size_t)t * 3] * 3, pos + (size_t)idx[(size_t)t * 3 + 1] * 3, pos + (size_t)idx[(size_t)t * 3 + 2] * 3, v0, e1, e2, tl,
               th);
    for (int a = 0; a < 3; a++) {
      lo[a] = tl[a] < lo[a] ? tl[a] : lo[a];
      hi[a] = hi[a] < th[a] ? th[a] : hi[a];
    }
  }
  for (int a = 0; a < 3; a++) {
    s[a][threadIdx.x] = lo[a];
    s[3 + a][threadIdx.x] = hi[a];
  }
  __syncthreads();
  for (uint32_t h = kBoxBlock / 2; h > 0; h >>= 1) {
    if (threadIdx.x < h)
      for (int a = 0; a < 3; a++) {
        const float l = s[a][threadIdx.x + h], u = s[3 + a][threadIdx.x + h];
        s[a][threadIdx.x] = l < s[a][threadIdx.x] ? l : s[a][threadIdx.x];
        s[3 + a][threadIdx.x] = s[3 + a][threadIdx.x] < u ? u : s[3 + a][threadIdx.x];
      }
    __syncthreads();
  }
  if (threadIdx.x < 6) partial[(size_t)blockIdx.x * 6 + threadIdx.x] = s[threadIdx.x][0];
}

__global__ __launch_bounds__(kBoxBlock) void k_refit_pad(const float* __restrict__ partial, uint32_t numPartials, uint32_t numTris, float* __restrict__ pad) {
  __shared__ float s[6][kBoxBlock];
  float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
  for (uint32_t b = threadIdx.x; b < numPartials; b += kBoxBlock)
    for (int a = 0; a < 3; a++) {
      const float l = partial[(size_t)b * 6 + a], u = partial[(size_t)b * 6 + 3 + a];
      lo[a] = l < lo[a] ? l : lo[a];
      hi[a] = hi[a] < u ? u : hi[a];
    }
  for (int a = 0; a < 3; a++) {
    s[a][threadIdx.x] = lo[a];
    s[3 + a][threadIdx.x] = hi[a];
  }
  __syncthreads();
  for (uint32_t h = kBoxBlock / 2; h > 0; h >>= 1) {
    if (threadIdx.x < h)
      for (int a = 0; a < 3; a++) {
        const float l = s[a][threadIdx.x + h], u = s[3 + a][threadIdx.x + h];
        s[a][threadIdx.x] = l < s[a][threadIdx.x] ? l : s[a][threadIdx.x];
        s[3 + a][threadIdx.x] = s[3 + a][threadIdx.x] < u ? u : s[3 + a][threadIdx.x];
      }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float l[3] = {s[0][0], s[1][0], s[2][0]}, u[3] = {s[3][0], s[4][0], s[5][0]};
    pad[0] = bvhPadOf(l, u, numTris != 0);
  }
}

__global__ __launch_bounds__(256) void k_refit_level(const BvhRefitNode* __restrict__ nodes, const uint32_t* __restrict__ order, uint32_t n,
                                                    BvhRec* recs, const float* __restrict__ pos, const uint32_t* __restrict__ idx, float* box,
                                                    float* __restrict__ childArea, const float* __restrict__ pad) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t self = order[i];
  bvhRefitNode(nodes[self], self, recs, pos, idx, box, childArea, pad[0]);
}

// the piece-tight instance (bvh.h "piece-tight refit"): the same node function with the regions; fixed-size loops only,
// no scratch
__global__ __launch_bounds__(256) void k_refit_level_pieces(const BvhRefitNode* __restrict__ nodes, const uint32_t* __restrict__ order, uint32_t n,
                                                           BvhRec* recs, const float* __restrict__ pos, const uint32_t* __restrict__ idx, float* box,
                                                           float* __restrict__ childArea, const float* __restrict__ pad,
                                                           const float* __restrict__ region) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t self = order[i];
  bvhRefitNodePieces(nodes[self], self, recs, pos, idx, box, childArea, pad[0], region);
}

// the regions, once per scene: a thread per plan node, a loop over its leaf children (the clipper's polygons live in
// scratch: this kernel runs once)
__global__ __launch_bounds__(256) void k_refit_regions(const BvhRefitNode* __restrict__ nodes, uint32_t n, const BvhRec* __restrict__ recs,
                                                      float* __restrict__ region) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bvhPieceRegionsOfNode(nodes[i], recs, region);
}

// positions (and normals) of the 128-byte shading records (api_scene.cpp sideUploads): three (position, normal, uv) vertices
// + material id; the uvs and the material id stay
__global__ __launch_bounds__(256) void k_refit_shade(float4* __restrict__ shade, const uint32_t* __restrict__ idx, const float* __restrict__ pos,
                                                    const float* __restrict__ nrm, uint32_t numTris) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= numTris) return;
  float* r = reinterpret_cast<float*>(shade + (size_t)t * kShadeRecF4);
  for (int k = 0; k < 3; k++) {
    const size_t vi = idx[(size_t)t * 3 + k];
    float* q = r + k * 8;
    q[0] = pos[vi * 3];
    q[1] = pos[vi * 3 + 1];
    q[2] = pos[vi * 3 + 2];
    if (nrm) {
      q[3] = nrm[vi * 3];
      q[4] = nrm[vi * 3 + 1];
      q[5] = nrm[vi * 3 + 2];
    }
  }
}

}  // namespace

void launchRefit(const RefitDev& R, BvhRec* recs, float4* shade, const uint32_t* indices, uint32_t numTris, const float* positions, const float* normals,
                 hipStream_t st) {
  const uint32_t nb = numTris ? (numTris + kBoxBlock - 1) / kBoxBlock : 1;
  const uint32_t blocks = nb < kRefitPartials ? nb : kRefitPartials;
  hipLaunchKernelGGL(k_refit_scene_box, dim3(blocks), dim3(kBoxBlock), 0, st, positions, indices, numTris, R.partial);
  hipLaunchKernelGGL(k_refit_pad, dim3(1), dim3(kBoxBlock), 0, st, R.partial, blocks, numTris, R.pad);
  for (size_t l = 0; l + 1 < R.levelStart.size(); l++) {
    const uint32_t a = R.levelStart[l], n = R.levelStart[l + 1] - a;
    if (!n) continue;
    if (R.region)
      hipLaunchKernelGGL(k_refit_level_pieces, dim3((n + 255) / 256), dim3(256), 0, st, R.nodes, R.levelOrder + a, n, recs, positions, indices, R.box,
                         R.childArea, R.pad, R.region);
    else
      hipLaunchKernelGGL(k_refit_level, dim3((n + 255) / 256), dim3(256), 0, st, R.nodes, R.levelOrder + a, n, recs, positions, indices, R.box, R.childArea, R.pad);
  }
  if (numTris) hipLaunchKernelGGL(k_refit_shade, dim3((numTris + 255) / 256), dim3(256), 0, st, shade, indices, positions, normals, numTris);
}

void launchRefitRegions(const RefitDev& R, const BvhRec* recs, float* region, hipStream_t st) {
  if (R.numNodes) hipLaunchKernelGGL(k_refit_regions, dim3((R.numNodes + 255) / 256), dim3(256), 0, st, R.nodes, R.numNodes, recs, region);
}

}  // namespace bdpt
