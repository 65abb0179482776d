// env_host.cpp — the host twins of environment lighting (include/bdpt.h "Environment lighting"): bdpt_host_env_table,
// bdpt_host_env_sample and bdpt_host_env_eval run env_light.h, the text the device kernels run, on the CPU.  No context,
// no device, no HIP: tests/sanitize/env_table_main.cpp builds this file alone.
#include "env_light.h"

using namespace bdpt;

namespace {
bool sizeOk(uint32_t w, uint32_t h) { return w >= 1 && h >= 1 && w <= kEnvMaxDim && h <= kEnvMaxDim; }
}  // namespace

extern "C" {

int bdpt_host_env_table(const float* map, uint32_t W, uint32_t H, uint32_t* q, uint32_t* cdf, uint64_t* rowCdf, float* outMax) {
  if (!map || !cdf || !rowCdf || !W || !H) return BDPT_E_INVALID;
  if (!sizeOk(W, H)) return BDPT_E_LIMIT;
  float m = 0.0f;
  for (uint32_t y = 0; y < H; y++) {
    const float sr = envSinRow(y, H);
    for (uint32_t x = 0; x < W; x++) {
      const float f = envTexelF(map + ((size_t)y * W + x) * 4, sr);
      if (f > m) m = f;
    }
  }
  uint64_t total = 0;
  for (uint32_t y = 0; y < H; y++) {
    const float sr = envSinRow(y, H);
    uint32_t run = 0;
    for (uint32_t x = 0; x < W; x++) {
      const size_t at = (size_t)y * W + x;
      const uint32_t qq = envQuantise(envTexelF(map + at * 4, sr), m);
      if (q) q[at] = qq;
      run += qq;
      cdf[at] = run;
    }
    total += run;
    rowCdf[y] = total;
  }
  if (outMax) *outMax = m;
  return BDPT_OK;
}

int bdpt_host_env_sample(const float* map, uint32_t W, uint32_t H, const uint32_t* cdf, const uint64_t* rowCdf, const uint32_t* seeds,
                         uint32_t n, bdpt_env_host_sample* out, uint32_t* seedsOut) {
  if (!map || !cdf || !rowCdf || !W || !H || (n && (!seeds || !out))) return BDPT_E_INVALID;
  if (!sizeOk(W, H)) return BDPT_E_LIMIT;
  const EnvTable T{map, W, H, cdf, rowCdf};
  for (uint32_t i = 0; i < n; i++) {
    uint32_t s = seeds[i];
    const EnvSample e = envSample(T, s);
    for (int k = 0; k < 3; k++) {
      out[i].dir[k] = e.dir[k];
      out[i].radiance[k] = e.radiance[k];
    }
    out[i].pdf = e.pdf;
    out[i].texel = e.texel;
    if (seedsOut) seedsOut[i] = s;
  }
  return BDPT_OK;
}

int bdpt_test_host_env_search(uint32_t W, uint32_t H, const uint32_t* cdf, const uint64_t* rowCdf, const float* r1, const float* r2, uint32_t n,
                              uint32_t* texels) {
  if (!cdf || !rowCdf || !W || !H || (n && (!r1 || !r2 || !texels))) return BDPT_E_INVALID;
  if (!sizeOk(W, H)) return BDPT_E_LIMIT;
  const EnvTable T{nullptr, W, H, cdf, rowCdf};
  const uint64_t total = rowCdf[H - 1];
  if (total == 0u) return BDPT_E_STATE;
  for (uint32_t i = 0; i < n; i++)  // draws are nextRand's: in [0, 1) (anything else has no defined conversion)
    if (!(r1[i] >= 0.0f && r1[i] < 1.0f && r2[i] >= 0.0f && r2[i] < 1.0f)) return BDPT_E_INVALID;
  for (uint32_t i = 0; i < n; i++) {
    uint32_t x, y;
    envSearch(T, total, r1[i], r2[i], x, y);
    texels[i] = y * W + x;
  }
  return BDPT_OK;
}

int bdpt_host_env_eval(const float* map, uint32_t W, uint32_t H, const uint32_t* cdf, const uint64_t* rowCdf, const float* dirs, uint32_t n,
                       bdpt_env_eval* out) {
  if (!map || !cdf || !rowCdf || !W || !H || (n && (!dirs || !out))) return BDPT_E_INVALID;
  if (!sizeOk(W, H)) return BDPT_E_LIMIT;
  const EnvTable T{map, W, H, cdf, rowCdf};
  for (uint32_t i = 0; i < n; i++) {
    const EnvEval e = envEval(T, dirs + (size_t)i * 4);
    for (int k = 0; k < 3; k++) out[i].radiance[k] = e.radiance[k];
    out[i].pdf = e.pdf;
    out[i].texel = e.texel;
    out[i].reserved[0] = out[i].reserved[1] = out[i].reserved[2] = 0u;
  }
  return BDPT_OK;
}

}  // extern "C"
