// env_light.h — environment lighting (bdpt_env_prepare / bdpt_env_query / bdpt_sky_query / bdpt_sky_mis_query /
// bdpt_host_env_*): the sampling table's per-texel arithmetic, the sampler, its pdf and the evaluation of a direction, shared
// by the device kernels (env_light.hip, sky.hip, sky_mis.hip) and the host entry points (env_host.cpp).  The arithmetic is
// the contract of include/bdpt.h "Environment lighting": fp32 and fp64 as written, no contraction (-ffp-contract=off on both
// sides), every operation in the order written here.  Plain C++ apart from the __host__ __device__ markers
// (texture_planes.h BDPT_HD).
//
// det_sincos2pi, det_acos, det_atan, atan2_WAR, normalize and nextRand are the texts of device_math.hpp / device_scene.hpp,
// which are device-only; they are restated here (namespace envl) so that the host runs them too.  tests/test_gpu_env.py
// holds bdpt_env_query(EVAL) to the G-buffer miss shader's envLookup bit for bit, which pins the restatement.
#pragma once
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "texture_planes.h"  // BDPT_HD

namespace bdpt {

constexpr uint32_t kEnvMaxDim = 16384;     // 1 <= W, H <= kEnvMaxDim: a row total is at most 2^30, the total at most 2^44
constexpr uint32_t kEnvRowScanChunk = 64;  // texels per pass of the row scan (one per lane of the row's wave)
constexpr uint32_t kEnvMarginalChunk = 64; // rows per pass of the marginal scan (one per lane of its one wave)
constexpr uint32_t kEnvNoTexel = 0xFFFFFFFFu;

// The table as the sampler reads it: the map (RGBA32F, caller memory), and the two integer prefix sums.
struct EnvTable {
  const float* map;
  uint32_t W, H;
  const uint32_t* cdf;     // [H][W]: inclusive prefix sum of q along each row
  const uint64_t* rowCdf;  // [H]: inclusive prefix sum of the row totals; rowCdf[H - 1] is the total
};

namespace envl {

constexpr float kPi = 3.14159265358979323846f;
constexpr float kInvPi = 0.318309886183790671538f;

BDPT_HD void sincos2pi(float u, float& s, float& c) {  // device_math.hpp det_sincos2pi
  float t = u * 4.0f;
  float q = floorf(t + 0.5f);
  float r = t - q;
  float a = r * 1.57079632679489661923f;
  float a2 = a * a;
  float sp = -1.0f / 5040.0f + a2 * (1.0f / 362880.0f);
  sp = 1.0f / 120.0f + a2 * sp;
  sp = -1.0f / 6.0f + a2 * sp;
  sp = 1.0f + a2 * sp;
  float sa = a * sp;
  float cp = 1.0f / 40320.0f + a2 * (-1.0f / 3628800.0f);
  cp = -1.0f / 720.0f + a2 * cp;
  cp = 1.0f / 24.0f + a2 * cp;
  cp = -0.5f + a2 * cp;
  float ca = 1.0f + a2 * cp;
  int qi = ((int)q) & 3;
  float s0 = (qi & 1) ? ca : sa;
  float c0 = (qi & 1) ? sa : ca;
  s = (qi & 2) ? -s0 : s0;
  c = ((qi == 1) || (qi == 2)) ? -c0 : c0;
}
BDPT_HD float acosPoly(float x) {  // device_math.hpp det_acos
  float ax = fabsf(x);
  if (ax > 1.0f) ax = 1.0f;
  float p = -0.0012624911f;
  p = 0.0066700901f + ax * p;
  p = -0.0170881256f + ax * p;
  p = 0.0308918810f + ax * p;
  p = -0.0501743046f + ax * p;
  p = 0.0889789874f + ax * p;
  p = -0.2145988016f + ax * p;
  p = 1.5707963050f + ax * p;
  float r = sqrtf(1.0f - ax) * p;
  return (x < 0.0f) ? (kPi - r) : r;
}
BDPT_HD float atanPoly(float z) {  // device_math.hpp det_atan
  float az = fabsf(z);
  bool inv = az > 1.0f;
  float w = inv ? (1.0f / az) : az;
  float w2 = w * w;
  float p = 0.0028662257f;
  p = -0.0161657367f + w2 * p;
  p = 0.0429096138f + w2 * p;
  p = -0.0752896400f + w2 * p;
  p = 0.1065626393f + w2 * p;
  p = -0.1420889944f + w2 * p;
  p = 0.1999355085f + w2 * p;
  p = -0.3333314528f + w2 * p;
  p = 1.0f + w2 * p;
  float r = w * p;
  if (inv) r = 1.57079632679489661923f - r;
  return (z < 0.0f) ? -r : r;
}
BDPT_HD float atan2War(float y, float x) {  // device_scene.hpp atan2_WAR
  if (x > 0.f)
    return atanPoly(y / x);
  else if (x < 0.f && y >= 0.f)
    return atanPoly(y / x) + kPi;
  else if (x < 0.f && y < 0.f)
    return atanPoly(y / x) - kPi;
  else if (x == 0.f && y > 0.f)
    return kPi / 2.f;
  else if (x == 0.f && y < 0.f)
    return -kPi / 2.f;
  return 0.f;
}
BDPT_HD float nextRand(uint32_t& s) {  // device_math.hpp nextRand
  s = 1664525u * s + 1013904223u;
  return (float)(s & 0x00FFFFFFu) / (float)0x01000000;
}
// float -> uint32 as the device's convert instruction does the plain cast of envLookup: toward zero, NaN and negatives 0,
// 2^32 and above 0xFFFFFFFF (the plain cast is undefined there in C++).
BDPT_HD uint32_t toU32(float x) {
  if (!(x > 0.0f)) return 0u;
  if (x >= 4294967296.0f) return 0xFFFFFFFFu;
  return (uint32_t)x;
}

}  // namespace envl

// ---- the table ----
// sinRow(y): the sine of the row centre's polar angle
BDPT_HD float envSinRow(uint32_t y, uint32_t H) {
  float s, c;
  envl::sincos2pi((((float)y + 0.5f) / (float)H) * 0.5f, s, c);
  return s;
}
// a channel as the table sees it: NaN and negatives 0, +inf FLT_MAX
BDPT_HD float envCleanChannel(float c) { return c > 0.0f ? (c < FLT_MAX ? c : FLT_MAX) : 0.0f; }
// f(x, y) = lum * sinRow from the texel's rgb: luminance (0.2126, 0.7152, 0.0722, summed left to right) of the cleaned
// channels.  So that a texel with any positive channel stays reachable, a luminance or a product that rounds to 0 counts
// as the smallest subnormal; so that the ratio f / m is defined, f is at most FLT_MAX.
BDPT_HD float envTexelF(const float* rgba, float sinRow) {
  const float r = envCleanChannel(rgba[0]), g = envCleanChannel(rgba[1]), b = envCleanChannel(rgba[2]);
  if (!(r > 0.0f || g > 0.0f || b > 0.0f)) return 0.0f;
  const float tiny = 1.40129846e-45f;
  float lum = (r * 0.2126f + g * 0.7152f) + b * 0.0722f;
  if (!(lum > 0.0f)) lum = tiny;
  float f = lum * sinRow;
  if (!(f > 0.0f)) f = sinRow > 0.0f ? tiny : 0.0f;
  return f < FLT_MAX ? f : FLT_MAX;
}
// q(x, y) in [0, 65536] from f and the map's maximum m (m >= f; m > 0 whenever f > 0)
BDPT_HD uint32_t envQuantise(float f, float m) {
  return f > 0.0f ? 1u + (uint32_t)(((double)f / (double)m) * 65535.0) : 0u;
}

// ---- the sampler ----
struct EnvSample {
  float dir[3];
  float radiance[3];
  float pdf;
  uint32_t texel;  // y * W + x
};

// the solid-angle density of texel probability q / total at polar sine st; evaluation order: the ratio in fp64, rounded
// once to fp32, times W, times H, over ((2 * (pi * pi)) * st)
BDPT_HD float envPdf(uint32_t q, uint64_t total, uint32_t W, uint32_t H, float st) {
  if (!(st > 0.0f) || total == 0u) return 0.0f;
  const float p = (float)((double)q / (double)total);
  return ((p * (float)W) * (float)H) / ((2.0f * (envl::kPi * envl::kPi)) * st);
}

// The table search of a sample, total > 0: the row from draw r1, the column from draw r2.  Every index comes from a search
// bounded by W and H, whatever the tables hold.  (bdpt_test_host_env_search runs it on a caller's draws.)
BDPT_HD void envSearch(const EnvTable& T, uint64_t total, float r1, float r2, uint32_t& x, uint32_t& y) {
  uint64_t t = (uint64_t)((double)r1 * (double)total);
  if (t > total - 1u) t = total - 1u;
  uint32_t lo = 0, hi = T.H - 1;  // the first y with rowCdf[y] > t
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (T.rowCdf[mid] > t)
      hi = mid;
    else
      lo = mid + 1;
  }
  y = lo;
  const uint32_t* row = T.cdf + (size_t)y * T.W;
  const uint32_t rowTotal = row[T.W - 1];
  uint32_t t2 = (uint32_t)((double)r2 * (double)rowTotal);
  if (rowTotal && t2 > rowTotal - 1u) t2 = rowTotal - 1u;
  lo = 0;
  hi = T.W - 1;  // the first x with cdf[y][x] > t2
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (row[mid] > t2)
      hi = mid;
    else
      lo = mid + 1;
  }
  x = lo;
}

// Exactly four draws, whatever happens.
BDPT_HD EnvSample envSample(const EnvTable& T, uint32_t& state) {
  const float r1 = envl::nextRand(state), r2 = envl::nextRand(state), r3 = envl::nextRand(state), r4 = envl::nextRand(state);
  EnvSample o;
  o.dir[0] = o.dir[1] = o.dir[2] = 0.0f;
  o.radiance[0] = o.radiance[1] = o.radiance[2] = 0.0f;
  o.pdf = 0.0f;
  o.texel = 0u;
  const uint64_t total = T.rowCdf[T.H - 1];
  if (total == 0u) return o;
  uint32_t x, y;
  envSearch(T, total, r1, r2, x, y);
  const uint32_t* row = T.cdf + (size_t)y * T.W;
  const uint32_t q = row[x] - (x ? row[x - 1] : 0u);
  const float u = ((float)x + r3) / (float)T.W, v = ((float)y + r4) / (float)T.H;
  float s, c, st, ct;
  envl::sincos2pi(u, s, c);
  envl::sincos2pi(v * 0.5f, st, ct);
  o.dir[0] = -st * s;
  o.dir[1] = ct;
  o.dir[2] = st * c;
  const float* px = T.map + ((size_t)y * T.W + x) * 4;
  o.radiance[0] = px[0];
  o.radiance[1] = px[1];
  o.radiance[2] = px[2];
  o.pdf = envPdf(q, total, T.W, T.H, st);
  o.texel = y * T.W + x;
  return o;
}

// ---- evaluation of a direction: envLookup's texel (device_scene.hpp), and the sampler's pdf for it ----
struct EnvEval {
  float radiance[3];
  float pdf;
  uint32_t texel;  // kEnvNoTexel: outside the map (radiance and pdf 0)
};

BDPT_HD EnvEval envEval(const EnvTable& T, const float* d) {
  const float inv = 1.0f / sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);  // normalize
  const float px = d[0] * inv, py = d[1] * inv, pz = d[2] * inv;
  const float u = (1.f + envl::atan2War(px, -pz) * envl::kInvPi) * 0.5f;
  const float v = envl::acosPoly(py) * envl::kInvPi;
  const uint32_t ex = envl::toU32(u * (float)T.W), ey = envl::toU32(v * (float)T.H);
  EnvEval o;
  o.radiance[0] = o.radiance[1] = o.radiance[2] = 0.0f;
  o.pdf = 0.0f;
  o.texel = kEnvNoTexel;
  if (ex < T.W && ey < T.H) {
    const float* t = T.map + ((size_t)ey * T.W + ex) * 4;
    o.radiance[0] = t[0];
    o.radiance[1] = t[1];
    o.radiance[2] = t[2];
    o.texel = ey * T.W + ex;
    const uint32_t* row = T.cdf + (size_t)ey * T.W;
    const uint32_t q = row[ex] - (ex ? row[ex - 1] : 0u);
    // the polar sine: 1 - py * py of the normalised direction, taken as px * px + pz * pz — the same quantity without the
    // cancellation, which near the poles (sine below about 0.03) costs more than the sampler's pdf can differ by
    const float s2 = px * px + pz * pz;
    o.pdf = envPdf(q, T.rowCdf[T.H - 1], T.W, T.H, sqrtf(s2 > 0.0f ? s2 : 0.0f));
  }
  return o;
}

}  // namespace bdpt

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "kernels.h"  // QueryRange, CompactList, SceneDev, LaunchGrids
namespace bdpt {
// The table's build (env_light.hip): three stream-ordered launches, no host read-back.  cdf / rowCdf: the context's
// (EnvState), writable here; maxBits: two words, [0] zero when the build starts and left zero, [1] the bits of m after it.
void launchEnvTable(const float* map, uint32_t W, uint32_t H, uint32_t* cdf, uint64_t* rowCdf, uint32_t* maxBits, hipStream_t st);
// bdpt_env_query (env_light.hip).  SAMPLE: one bdpt_env_sample (five float4) per bdpt_surface record and seed; EVAL: one
// bdpt_env_eval (two float4) per direction.
struct EnvQueryDev {
  EnvTable table;
  const float4* surf;     // SAMPLE: bdpt_surface records (six float4 each)
  const uint32_t* seeds;  // SAMPLE: one RNG state per item
  uint32_t* seedsOut;     // SAMPLE, optional: the state after the four draws
  const float4* dirs;     // EVAL
  float4* out;            // five (SAMPLE) or two (EVAL) float4 per item
  QueryRange range;
  CompactList compact;    // SAMPLE, optional: the rays with status == NONZERO
};
void launchEnvQuery(const EnvQueryDev& Q, bool evalMode, bool ggx, hipStream_t st);
// sky.hip: bdpt_sky_query (items are bdpt_surface records) and bdpt_sky_execute (items are the tile's pixels, read from the
// G-buffer).  `samples` table-sampled any-hit rays per alive item.
struct SkyDev {  // fields without a comment: the item source (device_item_source.hpp)
  EnvTable table;
  const float4* surf;         // posW, N, diffuse and prim are read
  const uint32_t* seeds;
  const uint8_t* alive;
  float4* color;
  uint32_t* counts;           // query, optional: traced and unoccluded samples per item
  uint32_t* seedsOut;         // query, optional: the state after 4 * samples draws (a dead item's: unchanged)
  const float4* gbPosition;
  const uint16_t* gbNormal;
  const uint16_t* gbDiffuse;
  const uint32_t* pix;
  float4* out;
  QueryRange range;
  float clampUpper;
  uint32_t samples;           // 1 .. 64
  uint32_t frameCount;        // execute
};
// `cursor`: as launchTraceRays (the context's two words: zero when the launch starts, left zero)
void launchSky(const SceneDev& S, const SkyDev& Q, bool gbuffer, unsigned long long* cursor, LaunchGrids& G, int numCUs, hipStream_t st);
// bdpt_bsdf_pdf_query (env_light.hip): out[i] = (fcos, pdf) of bdpt_surface record i toward dirs[i].xyz (device_bsdf_pdf.hpp);
// count (optional device word) caps cap
void launchBsdfPdfQuery(const float4* surf, uint32_t cap, const uint32_t* count, bool ggx, const float4* dirs, float4* out, hipStream_t st);
// sky_mis.hip: bdpt_sky_mis_query and bdpt_sky_mis_execute.  Per alive item and sample one table-sampled and one BSDF-sampled
// any-hit ray (`techniques` bit 0 / bit 1), weighted by the balance heuristic when both are on.
struct SkyMisDev {  // fields without a comment: the item source (device_item_source.hpp)
  EnvTable table;
  const float4* surf;           // posW, N, V, linearRoughness, diffuse, specular and prim are read
  const uint32_t* seeds;
  const uint8_t* alive;
  float4* color;
  uint32_t* counts;             // query, optional: traced and unoccluded terms per item (0 .. 2 * samples)
  uint32_t* seedsOut;           // query, optional: the state after (4 | 3 | 7) * samples draws (a dead item's: unchanged)
  const float4* gbPosition;
  const uint16_t* gbNormal;
  const uint16_t* gbDiffuse;
  const uint16_t* gbSpecRough;  // GGX only: specular = rgb, rough = a * a
  const uint32_t* pix;
  float4* out;
  QueryRange range;
  float camPos[3];              // execute, GGX: V = normalize(camPos - posW)
  float clampUpper;
  uint32_t samples;             // 1 .. 64
  uint32_t techniques;          // bit 0: table samples, bit 1: BSDF samples
  uint32_t frameCount;          // execute
};
// `cursor`: as launchSky
void launchSkyMis(const SceneDev& S, const SkyMisDev& Q, bool gbuffer, bool ggx, unsigned long long* cursor, LaunchGrids& G, int numCUs,
                  hipStream_t st);
}  // namespace bdpt
#endif
