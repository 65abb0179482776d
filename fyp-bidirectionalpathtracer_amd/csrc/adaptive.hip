// adaptive.hip — per-pixel running mean, variance and next-frame mask of adaptive sampling (bdpt_adaptive_update,
// bdpt_adaptive_reset).  The arithmetic is spelled out in include/bdpt.h "Adaptive sampling"; it is fp32 throughout, built
// with -ffp-contract=off and correctly rounded divide and sqrt (Makefile), so a float32 restatement matches it bit for bit.
//
// A wave takes aligned tiles of 8 x 8 pixels (16 x 16 for blockSize 16: four pixels per lane) in turn.  A lane folds its pixels'
// frame in, tests them for convergence, and the block decision is a __ballot over the tile: a lane's pixel stays active
// when any pixel of its aligned blockSize^2 block is unconverged.  Lanes past the right or bottom edge hold no pixel and
// count as converged, so a partial block decides on its real pixels only.
#include "kernels.h"

#include <algorithm>

#include "device_math.hpp"
#include "device_trace.hpp"
#include "launch.hpp"

namespace bdpt {

#define BD __device__ __forceinline__

BD float adaptiveLum(float4 v) { return (0.2126f * v.x + 0.7152f * v.y) + 0.0722f * v.z; }

// the update of one pixel: true when it has not converged
BD bool adaptivePixel(const AdaptiveDev& A, size_t pix) {
  float4 mu = A.mean[pix];
  float m2 = A.m2[pix];
  uint32_t n = A.count[pix];
  if (A.mask[pix] != 0 && n < A.maxSamples) {
    const float4 c = A.frame[pix];
    const float a = (float)n, b = (float)(n + 1u);
    float4 r;
    r.x = (a * mu.x + c.x) / b;  // accumulate_kernel's running mean
    r.y = (a * mu.y + c.y) / b;
    r.z = (a * mu.z + c.z) / b;
    r.w = (a * mu.w + c.w) / b;
    const float lc = adaptiveLum(c), lo = adaptiveLum(mu), ln = adaptiveLum(r);
    m2 = m2 + (lc - lo) * (lc - ln);
    mu = r;
    n = n + 1u;
    A.mean[pix] = mu;
    A.m2[pix] = m2;
    A.count[pix] = n;
  }
  bool converged = n >= A.maxSamples;
  if (!converged && n >= A.minSamples) {
    const float nf = (float)n;
    converged = sqrtf(m2 / (nf * (nf - 1.0f))) / (adaptiveLum(mu) + A.epsilon) <= A.threshold;
  }
  A.frame[pix] = mu;  // the pipeline's output shows the accumulated image
  return !converged;
}

// NSUB = 1: tiles of 8 x 8 (blockSize 1 to 8); NSUB = 4: tiles of 16 x 16 (blockSize 16), lane l holding pixel
// (l % 8, l / 8) of each 8 x 8 quarter
template <uint32_t NSUB>
__global__ __launch_bounds__(kWave) void adaptive_update_kernel(AdaptiveDev A, unsigned long long* __restrict__ scratch) {
  BDPT_ONE_WAVE_PER_GROUP();
  constexpr uint32_t T = (NSUB == 4u) ? 16u : 8u;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t B = A.blockSize;
  const uint32_t tilesX = (A.W + T - 1u) / T, numTiles = tilesX * ((A.H + T - 1u) / T);
  uint32_t nActive = 0;
  // (a capped grid: with one wave per tile, every 64 pixels would add an atomic pair on the two words below)
  for (uint32_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
    const uint32_t tx = tile % tilesX, ty = tile / tilesX;
    uint32_t x[NSUB], y[NSUB];
    bool real[NSUB];
    unsigned long long unconv[NSUB];
#pragma unroll
    for (uint32_t j = 0; j < NSUB; j++) {
      x[j] = tx * T + (j & 1u) * 8u + lane % 8u;
      y[j] = ty * T + (j >> 1) * 8u + lane / 8u;
      real[j] = x[j] < A.W && y[j] < A.H;
      const bool u = real[j] && adaptivePixel(A, (size_t)y[j] * A.W + x[j]);
      unconv[j] = __ballot(u);
    }
    // the lanes of this lane's block (B <= 8: a B x B square of the 8 x 8 tile, lane = row * 8 + column)
    bool keep = false;
    if (NSUB == 4u) {
      unsigned long long any = 0ull;
#pragma unroll
      for (uint32_t j = 0; j < NSUB; j++) any |= unconv[j];
      keep = any != 0ull;
    } else {
      const uint32_t bx0 = (lane % 8u) / B * B, by0 = (lane / 8u) / B * B;
      const unsigned long long row = ((1ull << B) - 1ull) << bx0;
      unsigned long long block = 0ull;
      for (uint32_t r = 0; r < B; r++) block |= row << ((by0 + r) * 8u);
      keep = (unconv[0] & block) != 0ull;
    }
#pragma unroll
    for (uint32_t j = 0; j < NSUB; j++) {
      if (real[j]) A.mask[(size_t)y[j] * A.W + x[j]] = keep ? 1u : 0u;
      nActive += (uint32_t)__popcll(__ballot(real[j] && keep));
    }
  }
  // `active`: the waves' counts summed in scratch[0]; the last wave to finish (scratch[1]) publishes the sum and leaves
  // both words zero for the next launch (no memset node: a captured graph is this one kernel)
  if (lane == 0) {
    if (nActive) atomicAdd(&scratch[0], (unsigned long long)nActive);
    __threadfence();
    if (atomicAdd(&scratch[1], 1ull) == (unsigned long long)gridDim.x - 1ull) {
      *A.active = (uint32_t)atomicExch(&scratch[0], 0ull);
      scratch[1] = 0ull;
    }
  }
}

__global__ void adaptive_reset_kernel(AdaptiveDev A) {
  const size_t n = (size_t)A.W * A.H;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    A.mean[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    A.m2[i] = 0.0f;
    A.count[i] = 0u;
    A.mask[i] = 1u;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *A.active = A.W * A.H;
}

void launchAdaptiveUpdate(const AdaptiveDev& A, unsigned long long* scratch, hipStream_t st) {
  const uint32_t T = (A.blockSize == 16u) ? 16u : 8u;
  const uint64_t tiles = (uint64_t)((A.W + T - 1u) / T) * ((A.H + T - 1u) / T);
  if (!tiles) return;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(tiles, 2048);
  if (T == 16u)
    launchWave(adaptive_update_kernel<4>, grid, st, A, scratch);
  else
    launchWave(adaptive_update_kernel<1>, grid, st, A, scratch);
}

void launchAdaptiveReset(const AdaptiveDev& A, hipStream_t st) {
  const uint64_t n = (uint64_t)A.W * A.H;
  if (!n) return;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(adaptive_reset_kernel, dim3(grid), dim3(256), 0, st, A);
}

}  // namespace bdpt
