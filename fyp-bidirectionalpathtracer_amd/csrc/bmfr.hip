// bmfr.hip — the reference's BMFR denoise pass as three HIP kernels for gfx950, over numPlanes images that share one
// G-buffer (bdpt_bmfr_execute and bdpt_bmfr_execute_motion: one image; bdpt_bmfr_execute_planes: up to
// BDPT_BMFR_MAX_PLANES; DESIGN.md "Denoised light groups").
//
//   bmfr_preprocess_kernel<MOTION>    Data/preprocess.ps.hlsl:33-165 (+ the three history blits of DenoisePass.cpp:180-182,
//                                     written into the other half of a ping-pong pair instead of copied afterwards)
//   bmfr_fit_kernel<IGNORE_LD, K>     Data/regressionCP.hlsl:100-500: one 256-thread workgroup per 32x32 block; the ten
//                                     feature columns of the working matrix (out_data) live in LDS (40 KiB, column-major so
//                                     a thread's four pixels are conflict-free), the normalised features (tmp_data) and the
//                                     colour columns of K planes in registers; the reference keeps out_data and tmp_data in
//                                     R32Float textures in device memory
//   bmfr_postprocess_kernel           Data/postprocess.ps.hlsl:22-91 (+ the two blits of DenoisePass.cpp:193-194)
//
// Geometry once, colour per plane.  Whatever reads positions and normals only is done once for all the images: the
// reprojection, the tap tests, accept, prevPixel and the position / normal history; feature scaling and the Householder
// reflectors of the ten feature columns; the postprocess taps and weights.  Whatever reads a colour is done per plane, with
// the shader's expressions in the shader's order, so that every image gets the bits the pass gives it alone.
//
// Arithmetic contract as everywhere else (DESIGN.md "Numerics"): the shader's own reduction pairing, no FMA
// contraction, correctly rounded divide/sqrt, so the parity tests can compare with the CPU checker bit for bit.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "kernels.h"

namespace bdpt {

#define BD __device__ __forceinline__

namespace {

constexpr int kBufferCount = 13, kFeatures = 10, kFeaturesNotScaled = 4, kBlockPixels = 1024, kLocal = 256, kBlockEdge = 32;
constexpr int kSub = kBlockPixels / kLocal;
__constant__ int kBlockOffsets[16][2] = {{-30, -30}, {-12, -22}, {-24, -2}, {-8, -16}, {-26, -24}, {-14, -4}, {-4, -28}, {-26, -16},
                                         {-4, -2},   {-24, -32}, {-10, -10}, {-18, -18}, {-12, -30}, {-32, -4}, {-2, -20}, {-22, -12}};

BD float4 loadHalf4(const uint16_t* p, size_t i) {
  const uint2 w = reinterpret_cast<const uint2*>(p)[i];
  return make_float4(f16_to_f32((uint16_t)(w.x & 0xffffu)), f16_to_f32((uint16_t)(w.x >> 16)), f16_to_f32((uint16_t)(w.y & 0xffffu)),
                     f16_to_f32((uint16_t)(w.y >> 16)));
}
BD int mirror(int index, int size) {
  if (index < 0)
    index = (index < 0 ? -index : index) - 1;
  else if (index >= size)
    index = 2 * size - index - 1;
  return index;
}
BD float hashRandom(uint32_t a) {
  a = (a + 0x7ed55d16u) + (a << 12);
  a = (a ^ 0xc761c23cu) ^ (a >> 19);
  a = (a + 0x165667b1u) + (a << 5);
  a = (a + 0xd3a2646cu) ^ (a << 9);
  a = (a + 0xfd7046c5u) + (a << 3);
  a = (a ^ 0xb55a4f09u) ^ (a >> 16);
  return (float)a / 4294967296.0f;
}
// the shader's int sum wraps before it reaches random(uint): uint32_t arithmetic, defined for every frame number
BD float addRandom(float value, uint32_t id, uint32_t sub, uint32_t featureBuffer, uint32_t frame) {
  return value + 0.01f * 2 *
                     (hashRandom(id + sub * kLocal + featureBuffer * kBlockEdge * kBlockEdge + frame * kBufferCount * kBlockEdge * kBlockEdge) -
                      0.5f);
}

// side `side` of plane k's slot in histNoisy / histFiltered (kernels.h BmfrDev)
BD float4* planeHist(float4* base, const BmfrDev& A, uint32_t k, uint32_t side) {
  return base + (size_t)(2u * k + side) * ((size_t)A.W * A.H);
}

}  // namespace

// MOTION (bdpt_bmfr_execute_motion): the reprojection and the position test use q = A.prevPos[i], where the pixel's surface
// point was in the previous frame, instead of its current position cp; everything else, the history write included, is
// the plain instance's.
template <bool MOTION>
__global__ __launch_bounds__(256) void bmfr_preprocess_kernel(BmfrDev A) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t n = A.W * A.H;
  if (i >= n) return;
  const int W = (int)A.W, H = (int)A.H;
  const int x = (int)(i % A.W), y = (int)(i / A.W);
  const float4 cp = A.curPos[i];
  const float4 q = MOTION ? A.prevPos[i] : cp;
  const float4 cn = loadHalf4(A.curNorm, i);
  const float posx = (float)x + 0.5f, posy = (float)y + 0.5f;
  const float texCx = posx / (float)W;
  const bool process = A.doPre && (A.full || !(texCx > 0.5f));
  // geometry: the reprojection and the four taps' tests, once
  float pfx = posx, pfy = posy;
  uint32_t storeAccept = 0;
  float totalWeight = 0;
  float wts[4] = {0, 0, 0, 0};
  uint32_t tap[4] = {0, 0, 0, 0};
  bool outside = false;
  if (process && A.frame > 0) {
    float c[4];
#pragma unroll
    for (int r = 0; r < 4; r++) c[r] = ((A.m[4 * r] * q.x + A.m[4 * r + 1] * q.y) + A.m[4 * r + 2] * q.z) + A.m[4 * r + 3];
    float ux = c[0] / c[3], uy = c[1] / c[3];
    ux = (ux + 1.0f) / 2.0f;
    uy = (1 - uy) / 2.0f;
    if (ux > 1.0f || ux < 0.0f || uy > 1.0f || uy < 0.0f) {
      outside = true;
    } else {
      pfx = ux * (float)A.W - 0.5f;
      pfy = uy * (float)A.H - 0.5f;
      const int ipx = ftoi(pfx), ipy = ftoi(pfy);  // pfx is a NaN for ux = 0/0, which passes the test above
      const float fx = pfx - (float)ipx, fy = pfy - (float)ipy;
      const float ox = 1.0f - fx, oy = 1.0f - fy;
      wts[0] = ox * oy;
      wts[1] = fx * oy;
      wts[2] = ox * fy;
      wts[3] = fx * fy;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int sx = ipx + (k & 1), sy = ipy + (k >> 1);
        if (sx >= 0 && sy >= 0 && sx < W && sy < H) {
          const uint32_t j = (uint32_t)sy * A.W + (uint32_t)sx;
          const float4 pp = A.prevPosR[j];
          const float dx = pp.x - q.x, dy = pp.y - q.y, dz = pp.z - q.z;
          const float pd = (dx * dx + dy * dy) + dz * dz;
          if (pd < 0.01f) {
            const float4 pn = A.prevNormR[j];
            const float ex = pn.x - cn.x, ey = pn.y - cn.y, ez = pn.z - cn.z;
            const float nd = (ex * ex + ey * ey) + ez * ez;
            if (nd < 1.0f) {
              storeAccept |= 1u << k;
              tap[k] = j;
              totalWeight += wts[k];
            }
          }
        }
      }
    }
  }
  if (process) {
    if (outside) {
      A.accept[i] = 0;
    } else {
      A.accept[i] = (uint8_t)storeAccept;
      A.prevPixel[i] = (uint32_t)f32_to_f16(pfx) | ((uint32_t)f32_to_f16(pfy) << 16);  // RG16Float
    }
  }
  // history for the next frame (DenoisePass.cpp:180-182), other half of the ping-pong pair; the noisy colours follow below
  A.prevNormW[i] = cn;
  A.prevPosW[i] = cp;
  // colours: per plane, from the plane's own history
  for (uint32_t p = 0; p < A.numPlanes; p++) {
    float4 cur = A.planes[p][i];
    if (process) {
      if (outside) {
        cur.w = 1.0f;
      } else {
        const float4* prevNoisyR = planeHist(A.histNoisy, A, p, A.read);
        float blendAlpha = 1.0f;
        float pr = 0, pg = 0, pb = 0, sampleSpp = 0;
#pragma unroll
        for (int k = 0; k < 4; k++)
          if (storeAccept & (1u << k)) {
            const float4 pd4 = prevNoisyR[tap[k]];
            sampleSpp += wts[k] * pd4.w;
            pr += wts[k] * pd4.x;
            pg += wts[k] * pd4.y;
            pb += wts[k] * pd4.z;
          }
        if (totalWeight > 0.0f) {
          pr /= totalWeight;
          pg /= totalWeight;
          pb /= totalWeight;
          sampleSpp /= totalWeight;
          blendAlpha = 1.0f / (sampleSpp + 1.0f);
          blendAlpha = blendAlpha > 0.2f ? blendAlpha : 0.2f;
        }
        float newSpp = 1.0f;
        if (blendAlpha < 1.0f) newSpp += sampleSpp;
        cur = make_float4(blendAlpha * cur.x + (1.0f - blendAlpha) * pr, blendAlpha * cur.y + (1.0f - blendAlpha) * pg,
                          blendAlpha * cur.z + (1.0f - blendAlpha) * pb, newSpp);
      }
      A.planes[p][i] = cur;
    }
    planeHist(A.histNoisy, A, p, 1u - A.read)[i] = cur;
  }
}

// v[i] (op)= v[i+128], +64, ... +2, then v[0] (op) v[1]: the shader's reduction, pairing preserved
template <int OP>
BD float blockTree(float v, float* sumVec, int tid) {
  sumVec[tid] = v;
  __syncthreads();
#pragma unroll
  for (int stride = 128; stride >= 2; stride >>= 1) {
    if (tid < stride) {
      const float a = sumVec[tid], b = sumVec[tid + stride];
      sumVec[tid] = OP == 0 ? a + b : (OP == 1 ? fmaxf(a, b) : fminf(a, b));
    }
    __syncthreads();
  }
  const float a = sumVec[0], b = sumVec[1];
  const float r = OP == 0 ? a + b : (OP == 1 ? fmaxf(a, b) : fminf(a, b));
  __syncthreads();
  return r;
}

// blockTree<0> for N columns at once: column c's partial sums in sumN[c * kLocal ..]; every column keeps blockTree's pairing
// (v[t] += v[t + stride], then v[0] + v[1]), the N * stride additions of a level are spread over the whole workgroup, and
// the columns share the level's barrier
template <int N>
BD void blockTreeSumN(const float (&v)[N], float (&r)[N], float* sumN, int tid) {
#pragma unroll
  for (int c = 0; c < N; c++) sumN[c * kLocal + tid] = v[c];
  __syncthreads();
#pragma unroll
  for (int stride = 128; stride >= 2; stride >>= 1) {
#pragma unroll
    for (int item = tid; item < N * stride; item += kLocal) {
      const int at = (item / stride) * kLocal + item % stride;
      const float a = sumN[at], b = sumN[at + stride];
      sumN[at] = a + b;
    }
    __syncthreads();
  }
#pragma unroll
  for (int c = 0; c < N; c++) {
    const float a = sumN[c * kLocal], b = sumN[c * kLocal + 1];
    r[c] = a + b;
  }
  __syncthreads();
}

// K: planes whose colour columns are carried through the ten steps together (3 K columns per tree pass); a workgroup
// takes its planes K at a time
template <bool IGNORE_LD, int K>
__global__ __launch_bounds__(256) void bmfr_fit_kernel(BmfrDev A, int horizontalBlocks) {
  constexpr int kCols = 3 * K;
  __shared__ float outS[kFeatures * kBlockPixels];  // the feature columns; after the factorisation column c = reflector c
  __shared__ float sumN[kCols * kLocal];            // (the feature trees use its first kLocal words)
  __shared__ float rfeat[kFeatures][kFeatures];     // R of the features: the shader's rmat[.][0..9]
  __shared__ float rcol[kCols][kFeatures];          // its rmat[.][10..12] for the planes in flight, one row per colour column
  __shared__ float stepUls[kFeatures];
  __shared__ int stepFirst[kFeatures];  // firstUpd of the step; -1: the step was skipped (rank dropped)
  __shared__ float bcast[2];
  const int tid = (int)threadIdx.x, group = (int)blockIdx.x;
  const int W = (int)A.W, H = (int)A.H;
  const uint32_t frame = A.frame;  // uint in the shader's constant buffer: frame % 16u stays inside the table
  const int offx = kBlockOffsets[frame % 16u][0], offy = kBlockOffsets[frame % 16u][1];
  const int bx = (group % horizontalBlocks) * kBlockEdge + offx, by = (group / horizontalBlocks) * kBlockEdge + offy;
  float tmp[kSub][kFeatures];
  uint32_t pix[kSub];  // the (mirrored) pixel each row loads; ~0u: outside the texture, loads give 0
#define OUT(index, buf) outS[(buf) * kBlockPixels + (index)]
#pragma unroll
  for (int s = 0; s < kSub; s++) {
    const int index = s * kLocal + tid;
    const int ux = mirror(bx + index % kBlockEdge, W), uy = mirror(by + index / kBlockEdge, H);
    // a frame narrower than the block offset is not covered by one reflection: such loads fall outside the
    // texture and return 0 in D3D
    const bool inside = ux >= 0 && uy >= 0 && ux < W && uy < H;
    const size_t i = inside ? (size_t)uy * W + ux : 0;
    pix[s] = inside ? (uint32_t)i : ~0u;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 p = inside ? A.curPos[i] : zero;
    const float4 nrm = inside ? loadHalf4(A.curNorm, i) : zero;
    tmp[s][0] = 1.0f;
    tmp[s][1] = nrm.x;
    tmp[s][2] = nrm.y;
    tmp[s][3] = nrm.z;
    tmp[s][4] = p.x;
    tmp[s][5] = p.y;
    tmp[s][6] = p.z;
    tmp[s][7] = p.x * p.x;
    tmp[s][8] = p.y * p.y;
    tmp[s][9] = p.z * p.z;
  }
  // scale features 4..9 to the block's range (regressionCP.hlsl:122-182)
#pragma unroll
  for (int fb = kFeaturesNotScaled; fb < kFeatures; fb++) {
    float mx = tmp[0][fb], mn = tmp[0][fb];
#pragma unroll
    for (int s = 1; s < kSub; s++) {
      mx = fmaxf(tmp[s][fb], mx);
      mn = fminf(tmp[s][fb], mn);
    }
    const float blockMax = blockTree<1>(mx, sumN, tid);
    const float blockMin = blockTree<2>(mn, sumN, tid);
    const bool wide = blockMax - blockMin > 1.0f;
#pragma unroll
    for (int s = 0; s < kSub; s++) tmp[s][fb] = wide ? (tmp[s][fb] - blockMin) / (blockMax - blockMin) : tmp[s][fb] - blockMin;
  }
#pragma unroll
  for (int fb = 0; fb < kFeatures; fb++)
#pragma unroll
    for (int s = 0; s < kSub; s++) OUT(s * kLocal + tid, fb) = tmp[s][fb];
  __syncthreads();

  // Householder QR over the 10 feature columns (regressionCP.hlsl:200-330 / 331-440); each step leaves what a colour
  // column needs from it: the reflector in its column of outS, firstUpd and uLengthSquared in stepFirst / stepUls
  float u[kSub];
  float uLengthSquared = 0.0f;
  int limit = 0;
  for (int col = 0; col < kFeatures; col++) {
    const int firstRow = IGNORE_LD ? limit + 1 : col + 1;
    float acc = 0.0f;
#pragma unroll
    for (int s = 0; s < kSub; s++) {
      const int index = s * kLocal + tid;
      const float v = OUT(index, col);
      u[s] = v;
      if (index >= firstRow) acc += v * v;
    }
    float vecLength = blockTree<0>(acc, sumN, tid);
    const int pivot = IGNORE_LD ? limit : col;
    float rValue = 0.0f;
    if (tid < pivot) {
      rValue = u[0];
    } else if (tid == pivot) {
      float uls = vecLength;
      vecLength = sqrtf(vecLength + u[0] * u[0]);
      u[0] -= vecLength;
      uls += u[0] * u[0];
      rValue = vecLength;
      bcast[0] = vecLength;
      bcast[1] = uls;
      OUT(tid, col) = u[0];  // the reflector stays in its column; the R value it replaces is in rfeat
    }
    if (tid == 0) stepFirst[col] = -1;
    __syncthreads();
    vecLength = bcast[0];
    uLengthSquared = bcast[1];
    if (IGNORE_LD) {
      if (vecLength > 0.01f) {
        limit++;
        if (tid < kFeatures) rfeat[tid][col] = rValue;
      } else {
        if (tid < kFeatures) rfeat[tid][col] = 0.0f;
        __syncthreads();  // bcast is rewritten by the next column's pivot thread
        continue;
      }
      if (uLengthSquared < 0.001f) {
        __syncthreads();
        continue;
      }
    } else {
      if (tid < kFeatures) rfeat[tid][col] = rValue;
    }
    const int firstUpd = IGNORE_LD ? limit - 1 : col;
    if (tid == 0) {
      stepFirst[col] = firstUpd;
      stepUls[col] = uLengthSquared;
    }
    for (int fb = col + 1; fb < kFeatures; fb++) {
      float cache[kSub];
      float dot = 0.0f;
#pragma unroll
      for (int s = 0; s < kSub; s++) {
        const int index = s * kLocal + tid;
        if (index >= firstUpd) {
          float v = OUT(index, fb);
          if (!IGNORE_LD && col == 0) v = addRandom(v, (uint32_t)tid, (uint32_t)s, (uint32_t)fb, frame);
          cache[s] = v;
          dot += v * u[s];
        }
      }
      const float dotV = blockTree<0>(dot, sumN, tid);
#pragma unroll
      for (int s = 0; s < kSub; s++) {
        const int index = s * kLocal + tid;
        if (index >= firstUpd) OUT(index, fb) = cache[s] - 2.0f * u[s] * dotV / uLengthSquared;
      }
    }
    __syncthreads();
  }

  for (uint32_t p0 = 0; p0 < A.numPlanes; p0 += K) {
    // the demodulated colours of planes p0 .. p0 + K - 1 (rows of a thread are its own: registers, not LDS)
    float cv[kCols][kSub];
    float spp[K][kSub];
#pragma unroll
    for (int k = 0; k < K; k++) {
      const bool live = p0 + k < A.numPlanes;
      // the write side of the noisy history: the copy of gCurNoisy made just before the dispatch (DenoisePass.cpp:180)
      const float4* noisyW = planeHist(A.histNoisy, A, live ? p0 + k : p0, 1u - A.read);
#pragma unroll
      for (int s = 0; s < kSub; s++) {
        const bool inside = live && pix[s] != ~0u;
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const float4 alb = inside ? loadHalf4(A.albedo, pix[s]) : zero;
        const float4 c = inside ? noisyW[pix[s]] : zero;
        cv[3 * k][s] = alb.x < 0.01f ? 0.0f : c.x / alb.x;
        cv[3 * k + 1][s] = alb.y < 0.01f ? 0.0f : c.y / alb.y;
        cv[3 * k + 2][s] = alb.z < 0.01f ? 0.0f : c.z / alb.z;
        spp[k][s] = c.w;
      }
    }
    // the reflectors applied to the colour columns, in the steps' order
    for (int col = 0; col < kFeatures; col++) {
      const int firstUpd = stepFirst[col];
      if (firstUpd < 0) continue;
      const float uls = stepUls[col];
#pragma unroll
      for (int s = 0; s < kSub; s++) u[s] = OUT(s * kLocal + tid, col);
      float dot[kCols], dotV[kCols];
#pragma unroll
      for (int c = 0; c < kCols; c++) {
        dot[c] = 0.0f;
#pragma unroll
        for (int s = 0; s < kSub; s++)
          if (s * kLocal + tid >= firstUpd) dot[c] += cv[c][s] * u[s];
      }
      blockTreeSumN<kCols>(dot, dotV, sumN, tid);
#pragma unroll
      for (int c = 0; c < kCols; c++)
#pragma unroll
        for (int s = 0; s < kSub; s++)
          if (s * kLocal + tid >= firstUpd) cv[c][s] = cv[c][s] - 2.0f * u[s] * dotV[c] / uls;
    }
    if (tid < kFeatures) {
#pragma unroll
      for (int c = 0; c < kCols; c++) rcol[c][tid] = cv[c][0];
    }
    __syncthreads();
    // back substitution (regressionCP.hlsl:332-352 / 441-455): 10 unknowns per colour column, in the order the shader's
    // barriers impose; one lane per column (the channels never mix)
    if (tid < kCols) {
      float* rc = rcol[tid];
      if (IGNORE_LD) {
        int lim = limit - 1;
        for (int i = kFeatures - 1; i >= 0; i--) {
          if (lim >= 0 && rfeat[lim][i] != 0.0f) {
            rc[i] = rc[lim] / rfeat[lim][i];
            lim--;
          } else {
            rc[i] = 0.0f;
          }
          for (int rowId = lim; rowId >= 0; rowId--) rc[rowId] -= rc[i] * rfeat[rowId][i];
        }
      } else {
        for (int i = kFeatures - 1; i >= 0; i--) {
          rc[i] /= rfeat[i][i];
          for (int rowId = i - 1; rowId >= 0; rowId--) rc[rowId] -= rc[i] * rfeat[rowId][i];
        }
      }
    }
    __syncthreads();
    // filtered colour = features . weights, re-modulated by albedo (regressionCP.hlsl:458-500)
#pragma unroll
    for (int k = 0; k < K; k++) {
      if (p0 + k >= A.numPlanes) break;
      float4* out = A.planes[p0 + k];
#pragma unroll
      for (int s = 0; s < kSub; s++) {
        const int index = s * kLocal + tid;
        float r = 0.0f, g = 0.0f, b = 0.0f;
#pragma unroll
        for (int col = 0; col < kFeatures; col++) {
          const float t = tmp[s][col];
          r += rcol[3 * k][col] * t;
          g += rcol[3 * k + 1][col] * t;
          b += rcol[3 * k + 2][col] * t;
        }
        const int ux = bx + index % kBlockEdge, uy = by + index / kBlockEdge;
        if (ux < 0 || uy < 0 || ux >= W || uy >= H) continue;
        const size_t i = (size_t)uy * W + ux;
        const float4 alb = loadHalf4(A.albedo, i);
        out[i] = make_float4(alb.x * (r < 0.0f ? 0.0f : r), alb.y * (g < 0.0f ? 0.0f : g), alb.z * (b < 0.0f ? 0.0f : b), alb.w * spp[k][s]);
      }
    }
    __syncthreads();  // rcol is rewritten by the next K planes
  }
#undef OUT
}

__global__ __launch_bounds__(256) void bmfr_postprocess_kernel(BmfrDev A) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t n = A.W * A.H;
  if (i >= n) return;
  const int W = (int)A.W, H = (int)A.H;
  const int x = (int)(i % A.W);
  const float texCx = ((float)x + 0.5f) / (float)W;
  const bool passThrough = !A.full && texCx > 0.5f;
  // geometry: the accepted taps and their weights, once
  float wts[4] = {0, 0, 0, 0};
  uint32_t tap[4] = {~0u, ~0u, ~0u, ~0u};  // ~0u: outside the frame, the tap reads 0
  uint32_t accept = 0;
  float totalWeight = 0.0f;
  if (!passThrough && A.frame > 0) {
    accept = A.accept[i];
    if (accept > 0) {
      const uint32_t pw = A.prevPixel[i];
      const float pfx = f16_to_f32((uint16_t)(pw & 0xffffu)), pfy = f16_to_f32((uint16_t)(pw >> 16));
      const int ipx = ftoi(pfx), ipy = ftoi(pfy);
      const float fx = pfx - (float)ipx, fy = pfy - (float)ipy;
      const float ox = 1.0f - fx, oy = 1.0f - fy;
      wts[0] = ox * oy;
      wts[1] = fx * oy;
      wts[2] = ox * fy;
      wts[3] = fx * fy;
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (accept & (1u << k)) {
          totalWeight += wts[k];
          const int sx = ipx + (k & 1), sy = ipy + (k >> 1);
          if (sx >= 0 && sy >= 0 && sx < W && sy < H) tap[k] = (uint32_t)sy * A.W + (uint32_t)sx;
        }
    }
  }
  for (uint32_t p = 0; p < A.numPlanes; p++) {
    const float4 f = A.planes[p][i];
    float4 res;
    if (passThrough) {
      res = f;
    } else {
      const float4* prevFilteredR = planeHist(A.histFiltered, A, p, A.read);
      float prev[3] = {0, 0, 0};
      float blendAlpha = 1.0f;
      if (accept > 0) {
#pragma unroll
        for (int k = 0; k < 4; k++)
          if (accept & (1u << k)) {
            float4 pv = make_float4(0, 0, 0, 0);
            if (tap[k] != ~0u) pv = prevFilteredR[tap[k]];
            prev[0] += wts[k] * pv.x;
            prev[1] += wts[k] * pv.y;
            prev[2] += wts[k] * pv.z;
          }
        if (totalWeight > 0.0f) {
          blendAlpha = 1.0f / f.w;
          blendAlpha = blendAlpha > 0.1f ? blendAlpha : 0.1f;
          prev[0] /= totalWeight;
          prev[1] /= totalWeight;
          prev[2] /= totalWeight;
        }
      }
      res = make_float4(blendAlpha * f.x + (1.0f - blendAlpha) * prev[0], blendAlpha * f.y + (1.0f - blendAlpha) * prev[1],
                        blendAlpha * f.z + (1.0f - blendAlpha) * prev[2], 1.0f);
    }
    A.planes[p][i] = res;                                    // "only curNoisy will be displayed" (DenoisePass.cpp:193)
    planeHist(A.histFiltered, A, p, 1u - A.read)[i] = res;  // DenoisePass.cpp:194
  }
}

namespace {
template <int K>
void launchFit(const BmfrDev& A, uint32_t flags, int w, int h, hipStream_t st) {
  if (flags & BDPT_BMFR_KEEP_LD_FEATURES)
    hipLaunchKernelGGL((bmfr_fit_kernel<false, K>), dim3((uint32_t)(w * h)), dim3(256), 0, st, A, w);
  else
    hipLaunchKernelGGL((bmfr_fit_kernel<true, K>), dim3((uint32_t)(w * h)), dim3(256), 0, st, A, w);
}
}  // namespace

// one launch per stage whatever numPlanes is
void launchBmfr(const BmfrDev& A, uint32_t flags, hipStream_t st) {
  const uint32_t n = A.W * A.H;
  if (!n || !A.numPlanes) return;
  const dim3 grid((n + 255u) / 256u), block(256);
  if (A.prevPos)
    hipLaunchKernelGGL(bmfr_preprocess_kernel<true>, grid, block, 0, st, A);
  else
    hipLaunchKernelGGL(bmfr_preprocess_kernel<false>, grid, block, 0, st, A);
  if (flags & BDPT_BMFR_REGRESSION) {
    const int bw = ((int)A.W + 31) / 32, bh = ((int)A.H + 31) / 32;
    int w = bw + 1;
    const int h = bh + 1;
    if (!A.full) w /= 2;  // DenoisePass.cpp:262: the reference fits the left half only
    if (w * h > 0) {
      // K = planes per pass over the ten steps (4 at most); fewer planes than that take the narrower instance
      if (A.numPlanes == 1)
        launchFit<1>(A, flags, w, h, st);
      else if (A.numPlanes == 2)
        launchFit<2>(A, flags, w, h, st);
      else
        launchFit<4>(A, flags, w, h, st);
    }
  }
  if (flags & BDPT_BMFR_POSTPROCESS) hipLaunchKernelGGL(bmfr_postprocess_kernel, grid, block, 0, st, A);
}

#undef BD
}  // namespace bdpt