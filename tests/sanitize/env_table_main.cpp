// Stand-alone host program for tests/test_env_cpu.py, built with -fsanitize=address,undefined,float-cast-overflow together
// with csrc/env_host.cpp: bdpt_host_env_table, bdpt_host_env_sample and bdpt_host_env_eval (the text of csrc/env_light.h
// that the device kernels run) on degenerate maps — NaN, infinite, negative and subnormal texels, an all-zero map, 1 x 1,
// sizes just past the scan chunks — with states that give the smallest and the largest draws, and with NaN, zero and
// infinite directions.  Nothing here may be undefined in C++ or reach outside an array: the device runs the same text.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "bdpt.h"
#include "env_light.h"

static int gFailures = 0;
static void check(bool ok, const char* what, const char* map) {
  if (!ok) {
    std::printf("%s: %s\n", map, what);
    gFailures++;
  }
}

static void run(const char* name, uint32_t W, uint32_t H, const std::vector<float>& map) {
  std::vector<uint32_t> q((size_t)W * H), cdf((size_t)W * H);
  std::vector<uint64_t> rowCdf(H);
  float m = -1.0f;
  check(bdpt_host_env_table(map.data(), W, H, q.data(), cdf.data(), rowCdf.data(), &m) == BDPT_OK, "table failed", name);
  uint64_t sum = 0;
  for (uint32_t v : q) {
    check(v <= 65536u, "q above 65536", name);
    sum += v;
  }
  check(sum == rowCdf[H - 1], "sum q != total", name);
  check(m >= 0.0f && m <= 3.4028234663852886e38f, "m not in [0, FLT_MAX]", name);
  // states: whose first draws are 0 and 1 - 2^-24 (the LCG inverted), and a spread of others
  std::vector<uint32_t> seeds;
  const uint32_t inv = 4276115653u;
  for (uint32_t hi = 0; hi < 4; hi++) {
    seeds.push_back((((hi << 24) | 0u) - 1013904223u) * inv);
    seeds.push_back((((hi << 24) | 0xFFFFFFu) - 1013904223u) * inv);
  }
  for (uint32_t i = 0; i < 4096; i++) seeds.push_back(i * 2654435761u + 12345u);
  std::vector<bdpt_env_host_sample> out(seeds.size());
  std::vector<uint32_t> after(seeds.size());
  check(bdpt_host_env_sample(map.data(), W, H, cdf.data(), rowCdf.data(), seeds.data(), (uint32_t)seeds.size(), out.data(), after.data()) == BDPT_OK,
        "sample failed", name);
  std::vector<float> dirs;
  for (size_t i = 0; i < out.size(); i++) {
    uint32_t s = seeds[i];
    for (int k = 0; k < 4; k++) s = 1664525u * s + 1013904223u;
    check(after[i] == s, "not four draws", name);
    check(out[i].texel < W * H, "texel out of range", name);
    check(sum == 0 ? out[i].pdf == 0.0f : q[out[i].texel] > 0, "an unlit texel was drawn", name);
    check(!(out[i].pdf < 0.0f) && !std::isnan(out[i].pdf), "pdf negative or NaN", name);
    for (int k = 0; k < 3; k++) dirs.push_back(out[i].dir[k]);
    dirs.push_back(0.0f);
  }
  {  // the search on draws given directly: the smallest and the largest draw in every pairing; draws outside [0, 1) are refused
    const float top = 16777215.0f / 16777216.0f, ds[] = {0.0f, top, 0.5f, 1.0f / 16777216.0f};
    std::vector<float> a, b;
    for (float p : ds)
      for (float r : ds) a.push_back(p), b.push_back(r);
    std::vector<uint32_t> tex(a.size(), 0u);
    const int rc = bdpt_test_host_env_search(W, H, cdf.data(), rowCdf.data(), a.data(), b.data(), (uint32_t)a.size(), tex.data());
    check(rc == (sum == 0 ? BDPT_E_STATE : BDPT_OK), "search: wrong return code", name);
    for (uint32_t t : tex) check(t < W * H && (sum == 0 || q[t] > 0), "search: texel out of range or unlit", name);
    for (float bad : {1.0f, -1e-30f, NAN, INFINITY, 2.0f}) {
      const float g = 0.25f;
      uint32_t one = 7u;
      check(sum == 0 || (bdpt_test_host_env_search(W, H, cdf.data(), rowCdf.data(), &bad, &g, 1, &one) == BDPT_E_INVALID &&
                         bdpt_test_host_env_search(W, H, cdf.data(), rowCdf.data(), &g, &bad, 1, &one) == BDPT_E_INVALID && one == 7u),
            "search: a draw outside [0, 1) was not refused", name);
    }
  }
  const float odd[] = {0.0f, -0.0f, 1.0f, -1.0f, NAN, INFINITY, -INFINITY, 1e-45f, 3.4e38f, -3.4e38f, 1e-30f};
  for (float a : odd)
    for (float b : odd)
      for (float c : odd) {
        dirs.push_back(a);
        dirs.push_back(b);
        dirs.push_back(c);
        dirs.push_back(NAN);
      }
  const uint32_t nd = (uint32_t)(dirs.size() / 4);
  std::vector<bdpt_env_eval> ev(nd);
  check(bdpt_host_env_eval(map.data(), W, H, cdf.data(), rowCdf.data(), dirs.data(), nd, ev.data()) == BDPT_OK, "eval failed", name);
  for (const bdpt_env_eval& e : ev) {
    check(e.texel == 0xFFFFFFFFu || e.texel < W * H, "eval texel out of range", name);
    check(!(e.pdf < 0.0f) && !std::isnan(e.pdf), "eval pdf negative or NaN", name);
    if (e.texel == 0xFFFFFFFFu) check(e.pdf == 0.0f && e.radiance[0] == 0.0f && e.radiance[1] == 0.0f && e.radiance[2] == 0.0f, "outside the map but not zero", name);
  }
}

static std::vector<float> filled(uint32_t W, uint32_t H, float r, float g, float b) {
  std::vector<float> m((size_t)W * H * 4);
  for (size_t i = 0; i < (size_t)W * H; i++) {
    m[i * 4] = r;
    m[i * 4 + 1] = g;
    m[i * 4 + 2] = b;
    m[i * 4 + 3] = 1.0f;
  }
  return m;
}

int main() {
  const float vals[] = {NAN, INFINITY, -INFINITY, -1.0f, 0.0f, -0.0f, 1e-45f, 1e-40f, 3.4e38f, 1.0f, 1e-20f, 1e6f};
  const uint32_t nv = (uint32_t)(sizeof(vals) / sizeof(vals[0]));
  {  // every pair of odd values as (r, g), b cycling
    std::vector<float> m((size_t)nv * nv * 4);
    for (uint32_t y = 0; y < nv; y++)
      for (uint32_t x = 0; x < nv; x++) {
        float* t = &m[((size_t)y * nv + x) * 4];
        t[0] = vals[x];
        t[1] = vals[y];
        t[2] = vals[(x + y) % nv];
        t[3] = NAN;
      }
    run("odd values", nv, nv, m);
  }
  run("all zero", 4, 3, filled(4, 3, 0.0f, 0.0f, 0.0f));
  run("all NaN", 3, 2, filled(3, 2, NAN, NAN, NAN));
  run("all negative", 3, 2, filled(3, 2, -1.0f, -INFINITY, -0.0f));
  run("all inf", 2, 2, filled(2, 2, INFINITY, INFINITY, INFINITY));
  run("all subnormal", 5, 3, filled(5, 3, 1e-45f, 0.0f, 1e-45f));
  run("1x1", 1, 1, filled(1, 1, 1.0f, 2.0f, 3.0f));
  run("1x1 zero", 1, 1, filled(1, 1, 0.0f, 0.0f, 0.0f));
  run("past the row chunk", bdpt::kEnvRowScanChunk + 1, 2, filled(bdpt::kEnvRowScanChunk + 1, 2, 0.5f, 0.5f, 0.5f));
  run("past the marginal chunk", 2, bdpt::kEnvMarginalChunk + 1, filled(2, bdpt::kEnvMarginalChunk + 1, 0.5f, 0.5f, 0.5f));
  {  // one sun among dark texels
    std::vector<float> m = filled(64, 32, 1e-3f, 1e-3f, 1e-3f);
    m[((size_t)9 * 64 + 41) * 4] = 1e6f;
    run("sun", 64, 32, m);
  }
  std::vector<uint32_t> w(4);
  std::vector<uint64_t> r(4);
  const std::vector<float> one = filled(1, 1, 1.0f, 1.0f, 1.0f);
  if (bdpt_host_env_table(one.data(), 16385, 1, nullptr, w.data(), r.data(), nullptr) != BDPT_E_LIMIT) {
    std::printf("a width past the limit must give BDPT_E_LIMIT\n");
    gFailures++;
  }
  std::printf("env table run finished failures=%d\n", gFailures);
  return gFailures ? 1 : 0;
}
