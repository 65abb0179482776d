// env_light.hip — the environment map's sampling table on the device (bdpt_env_prepare), bdpt_env_query and
// bdpt_bsdf_pdf_query.
//
// The table is a discrete distribution over the texels of the lat-long map, exact in integers (include/bdpt.h
// "Environment lighting"; the per-texel arithmetic is env_light.h, which bdpt_host_env_table runs on the CPU).  Three
// stream-ordered launches, no host read-back and no memset: the maximum's word is zero between builds (the last kernel
// hands the maximum over and leaves the word zero, as the persistent kernels leave their cursor):
//   env_max_kernel       f per texel, the map's maximum by an unsigned atomicMax on the float's bits (f >= 0, so the bits
//                        order as the floats do): one wave per row, one atomic per wave
//   env_row_scan_kernel  q per texel and its inclusive prefix sum along the row: one wave per row, kEnvRowScanChunk texels
//                        per pass, a wave scan in uint32 and the running total carried from pass to pass
//   env_marginal_kernel  the inclusive prefix sum of the H row totals in uint64: one wave, kEnvMarginalChunk rows per pass;
//                        then maxBits[1] = maxBits[0] (what bdpt_get_env_info reads) and maxBits[0] = 0
// Integer sums and an order-free maximum: no result depends on the order the waves run in.
//
// bdpt_env_query has no traversal, so no persistent grid: one lane per item on a dense grid of one-wave workgroups, as
// light_query.hip.  The sampler and the evaluation are env_light.h's; the value is written with the device functions the
// pass runs (saturate, directIfVisible).  bdpt_bsdf_pdf_query (bsdf_pdf_kernel, beside the sample kernel) is the same kind
// of launch: the BSDF's fcos and sampling density toward a caller's direction (device_bsdf_pdf.hpp), for MIS.
#include "kernels.h"

#include "device_bsdf_pdf.hpp"
#include "device_math.hpp"
#include "device_query.hpp"
#include "device_trace.hpp"  // BDPT_ONE_WAVE_PER_GROUP
#include "env_light.h"
#include "launch.hpp"

namespace bdpt {

namespace {
// inclusive prefix sum over the wave's 64 lanes
__device__ __forceinline__ uint32_t waveScan32(uint32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)v, d);
    if (lane >= d) v += o;
  }
  return v;
}
__device__ __forceinline__ uint64_t waveScan64(uint64_t v, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d);
    if (lane >= d) v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}
}  // namespace

__global__ __launch_bounds__(kWave) void env_max_kernel(const float* __restrict__ map, uint32_t W, uint32_t H, uint32_t* maxBits) {
  BDPT_ONE_WAVE_PER_GROUP();
  const uint32_t y = blockIdx.x;
  if (y >= H) return;
  const int lane = (int)(threadIdx.x & 63u);
  const float sr = envSinRow(y, H);
  const float4* row = reinterpret_cast<const float4*>(map) + (size_t)y * W;
  float m = 0.0f;
  for (uint32_t x = (uint32_t)lane; x < W; x += (uint32_t)kWave) {
    const float4 t = row[x];
    const float rgba[4] = {t.x, t.y, t.z, t.w};
    const float f = envTexelF(rgba, sr);
    if (f > m) m = f;
  }
  uint32_t bits = __float_as_uint(m);
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)bits, d);
    bits = o > bits ? o : bits;
  }
  if (lane == 0 && bits) atomicMax(maxBits, bits);
}

__global__ __launch_bounds__(kWave) void env_row_scan_kernel(const float* __restrict__ map, uint32_t W, uint32_t H,
                                                             const uint32_t* __restrict__ maxBits, uint32_t* __restrict__ cdf) {
  BDPT_ONE_WAVE_PER_GROUP();
  const uint32_t y = blockIdx.x;
  if (y >= H) return;
  const int lane = (int)(threadIdx.x & 63u);
  const float sr = envSinRow(y, H);
  const float m = __uint_as_float(*maxBits);
  const float4* row = reinterpret_cast<const float4*>(map) + (size_t)y * W;
  uint32_t* out = cdf + (size_t)y * W;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < W; base += kEnvRowScanChunk) {  // wave-uniform
    const uint32_t x = base + (uint32_t)lane;
    uint32_t q = 0;
    if (x < W) {
      const float4 t = row[x];
      const float rgba[4] = {t.x, t.y, t.z, t.w};
      q = envQuantise(envTexelF(rgba, sr), m);
    }
    const uint32_t incl = waveScan32(q, lane);
    if (x < W) out[x] = carry + incl;
    carry += (uint32_t)__shfl((int)incl, kWave - 1);
  }
}

__global__ __launch_bounds__(kWave) void env_marginal_kernel(const uint32_t* __restrict__ cdf, uint32_t W, uint32_t H,
                                                             uint64_t* __restrict__ rowCdf, uint32_t* maxBits) {
  BDPT_ONE_WAVE_PER_GROUP();
  if (blockIdx.x != 0) return;
  const int lane = (int)(threadIdx.x & 63u);
  uint64_t carry = 0;
  for (uint32_t base = 0; base < H; base += kEnvMarginalChunk) {  // wave-uniform
    const uint32_t y = base + (uint32_t)lane;
    const uint64_t rowTotal = y < H ? (uint64_t)cdf[(size_t)y * W + (W - 1)] : 0ull;
    const uint64_t incl = waveScan64(rowTotal, lane);
    if (y < H) rowCdf[y] = carry + incl;
    carry += ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(incl >> 32), kWave - 1) << 32) | (uint32_t)__shfl((int)(uint32_t)incl, kWave - 1);
  }
  if (lane == 0) {  // the row scan, the word's last reader, is behind this launch in the stream
    maxBits[1] = maxBits[0];
    maxBits[0] = 0u;
  }
}

void launchEnvTable(const float* map, uint32_t W, uint32_t H, uint32_t* cdf, uint64_t* rowCdf, uint32_t* maxBits, hipStream_t st) {
  static_assert(kEnvRowScanChunk == (uint32_t)kWave && kEnvMarginalChunk == (uint32_t)kWave, "a pass is one texel / one row per lane");
  launchWave(env_max_kernel, H, st, map, W, H, maxBits);
  launchWave(env_row_scan_kernel, H, st, map, W, H, (const uint32_t*)maxBits, cdf);
  launchWave(env_marginal_kernel, 1u, st, (const uint32_t*)cdf, W, H, rowCdf, maxBits);
}

namespace {
// bdpt_env_sample: five float4 per item, (org, tmin) (dir, 1e38) (radiance, pdf) (value, texel) (status, 0, 0, 0).  Reads the
// record's posW, N, linearRoughness, diffuse and prim, and for GGX also V and specular.
template <bool GGX, bool COMPACT>
__device__ __forceinline__ void envSampleLane(const EnvQueryDev& Q) {
  uint32_t i, n;
  if (queryLanePast<COMPACT>(Q.range.cap, Q.range.count, i, n)) return;
  const bool act = i < n;
  bool emit = false;
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float4 q0 = zero, q1 = zero;
  if (act) {
    uint32_t seed = Q.seeds[i];
    const EnvSample e = envSample(Q.table, seed);  // the four draws, also for a record that is a miss
    if (Q.seedsOut) Q.seedsOut[i] = seed;
    const float4* rec = Q.surf + (size_t)i * 6;
    float4 q2 = zero, q3 = zero, q4 = zero;
    if (__float_as_int(rec[5].w) >= 0) {
      const float4 p = rec[0], nr = rec[1], dif = rec[3];
      const f3 dir = mk(e.dir[0], e.dir[1], e.dir[2]), rad = mk(e.radiance[0], e.radiance[1], e.radiance[2]);
      const f3 N = mk(nr.x, nr.y, nr.z), diffuse = mk(dif.x, dif.y, dif.z);
      f3 value = mk(0);
      if (e.pdf != 0.0f) {
        if (GGX) {
          const float4 v = rec[2], sp = rec[4];
          value = directIfVisible<true>(1.0f, dir, rad, N, mk(v.x, v.y, v.z), diffuse, mk(sp.x, sp.y, sp.z), nr.w * nr.w) / e.pdf;
        } else {
          const float NdotL = saturate(dot(N, dir));
          value = (((NdotL * rad) * diffuse) / kPi) / e.pdf;
        }
      }
      const uint32_t status = allZero(value) ? 0u : BDPT_ENV_STATUS_NONZERO;
      emit = status != 0u;
      q0 = make_float4(p.x, p.y, p.z, Q.range.minT);
      q1 = make_float4(dir.x, dir.y, dir.z, 1e+38f);
      q2 = make_float4(rad.x, rad.y, rad.z, e.pdf);
      q3 = make_float4(value.x, value.y, value.z, __uint_as_float(e.texel));
      q4 = make_float4(__uint_as_float(status), 0.0f, 0.0f, 0.0f);
    }
    float4* o = Q.out + (size_t)i * 5;
    o[0] = q0;
    o[1] = q1;
    o[2] = q2;
    o[3] = q3;
    o[4] = q4;
  }
  if (COMPACT) compactAppend(Q.compact, Q.range.cap, emit, i, q0, q1);
}
}  // namespace

template <bool GGX, bool COMPACT>
__global__ __launch_bounds__(kWave) void env_sample_kernel(EnvQueryDev Q) {
  BDPT_ONE_WAVE_PER_GROUP();
  envSampleLane<GGX, COMPACT>(Q);
}

// bdpt_bsdf_pdf_query: one float4 per item, (fcos, pdf) of the record toward dirs[i].xyz (bsdfFcosPdf); zeros for a record
// with prim < 0.  Reads the record's N, V, linearRoughness, diffuse, specular and prim only.
template <bool GGX>
__global__ __launch_bounds__(kWave) void bsdf_pdf_kernel(const float4* __restrict__ surf, uint32_t cap, const uint32_t* count,
                                                         const float4* __restrict__ dirs, float4* __restrict__ out) {
  BDPT_ONE_WAVE_PER_GROUP();
  uint32_t i;
  if (queryLanePast(cap, count, i)) return;
  const float4* r = surf + (size_t)i * 6;
  f3 fcos = mk(0);
  float pdf = 0.0f;
  if (__float_as_int(r[5].w) >= 0) {
    const float4 n = r[1], v = r[2], dif = r[3], spec = r[4], l = dirs[i];
    bsdfFcosPdf<GGX>(mk(l.x, l.y, l.z), mk(n.x, n.y, n.z), mk(v.x, v.y, v.z), mk(dif.x, dif.y, dif.z), mk(spec.x, spec.y, spec.z),
                     n.w * n.w, fcos, pdf);
  }
  out[i] = make_float4(fcos.x, fcos.y, fcos.z, pdf);
}

// bdpt_env_eval: two float4 per item, (radiance, pdf) (texel, 0, 0, 0)
__global__ __launch_bounds__(kWave) void env_eval_kernel(EnvQueryDev Q) {
  BDPT_ONE_WAVE_PER_GROUP();
  uint32_t i;
  if (queryLanePast(Q.range.cap, Q.range.count, i)) return;
  const float4 d = Q.dirs[i];
  const float dir[3] = {d.x, d.y, d.z};
  const EnvEval e = envEval(Q.table, dir);
  float4* o = Q.out + (size_t)i * 2;
  o[0] = make_float4(e.radiance[0], e.radiance[1], e.radiance[2], e.pdf);
  o[1] = make_float4(__uint_as_float(e.texel), 0.0f, 0.0f, 0.0f);
}

void launchEnvQuery(const EnvQueryDev& Q, bool evalMode, bool ggx, hipStream_t st) {
  if (!Q.range.cap) return;
  const uint32_t g = wavesFor(Q.range.cap);
  if (evalMode) {
    launchWave(env_eval_kernel, g, st, Q);
    return;
  }
  withFlag(ggx, [&](auto GGX) {
    withFlag(Q.compact.rays != nullptr, [&](auto COMPACT) { launchWave(env_sample_kernel<GGX, COMPACT>, g, st, Q); });
  });
}

void launchBsdfPdfQuery(const float4* surf, uint32_t cap, const uint32_t* count, bool ggx, const float4* dirs, float4* out, hipStream_t st) {
  if (!cap) return;
  withFlag(ggx, [&](auto GGX) { launchWave(bsdf_pdf_kernel<GGX>, wavesFor(cap), st, surf, cap, count, dirs, out); });
}

}  // namespace bdpt
