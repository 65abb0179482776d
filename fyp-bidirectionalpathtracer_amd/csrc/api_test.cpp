// api_test.cpp — the test hooks of the C ABI (include/bdpt.h "test hooks"): one kernel or one device function on a
// caller's host arrays.  But for bdpt_test_skin_kernel / bdpt_test_morph_kernel, which enqueue the deformation pass on the
// caller's stream, every one allocates its temporaries, launches on the null stream, synchronises the device and copies
// back before it returns, so none may be captured; the temporaries go with the DevPool on every way out.
#include <vector>

#include "api_common.hpp"
#include "scene_bvh.h"

using namespace bdpt;

namespace {
// bdpt_test_skin_kernel and bdpt_test_morph_kernel: the pass alone, with the palettes (and weights) of the last update
int testDeformKernel(bdpt_ctx* c, bool morph, uint32_t path, void* stream) {
  if (!c || path > (uint32_t)kSkinPathLds) return BDPT_E_INVALID;
  if (!c->scene.have || !(morph ? c->scene.skin.morph.have : c->scene.skin.have)) {
    fail(c, morph ? "test_morph_kernel: no morph (bdpt_set_morph first)" : "test_skin_kernel: no skin (bdpt_set_skin first)");
    return BDPT_E_STATE;
  }
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = orderAfterLast(c, st)) return rc;
  const SkinState& K = c->scene.skin;  // (palette[k] is null where the context has no skin, or its skin no normals)
  launchDeform(morph ? &K.morph.dev : nullptr, K.morph.weights, K.have ? &K.dev : nullptr, K.palette[0], K.palette[1], (int)path, st);
  HIPCHK(c, hipGetLastError());
  c->lastStream = st;
  return BDPT_OK;
}
}  // namespace

extern "C" {

int bdpt_test_skin_kernel(bdpt_ctx* c, uint32_t path, void* stream) { return testDeformKernel(c, false, path, stream); }
int bdpt_test_morph_kernel(bdpt_ctx* c, uint32_t path, void* stream) { return testDeformKernel(c, true, path, stream); }

// Test hook: which builder the host-only hash / check hooks (bdpt_bvh_build_hash, bdpt_bvh_build_check, bdpt_host_bvh_*)
// use for the binary tree: device >= 0 the device implementation on that device, < 0 the host code (the default).
int bdpt_test_tree_builder(int device) {
  static BvhDeviceBuild* sBuild = nullptr;
  bvhSetDefaultBackend(BvhBackend());
  if (sBuild) bvhDeviceBuildEnd(sBuild);
  sBuild = nullptr;
  if (device < 0) return BDPT_OK;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device >= count) return BDPT_E_HIP;
  sBuild = bvhDeviceBuildBegin(device);
  BvhBackend treeOnly;
  treeOnly.user = sBuild;
  treeOnly.buildTree = buildBinaryTreeOnDevice;
  bvhSetDefaultBackend(treeOnly);
  return BDPT_OK;
}

int bdpt_test_rng(bdpt_ctx* c, const uint32_t* val0, const uint32_t* val1, uint32_t n, uint32_t draws, uint32_t* out_states,
                  float* out_floats) {
  if (!c || !val0 || !val1 || !out_states || !out_floats) return BDPT_E_INVALID;
  ENTER(c);
  DevPool pool;
  const uint32_t *d0, *d1;
  uint32_t* ds;
  float* df;
  int rc;
  if ((rc = devUpload(c, pool, &d0, val0, n)) || (rc = devUpload(c, pool, &d1, val1, n)) ||
      (rc = devAlloc(c, pool, &ds, (size_t)n * draws)) || (rc = devAlloc(c, pool, &df, (size_t)n * draws)))
    return rc;
  launchTestRng(d0, d1, n, draws, ds, df, nullptr);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out_states, ds, (size_t)n * draws * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out_floats, df, (size_t)n * draws * 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    fail(c, hipGetErrorString(e));
    return BDPT_E_HIP;
  }
  return BDPT_OK;
}

int bdpt_test_trace(bdpt_ctx* c, const float* rays, uint32_t n, int mode, int32_t* out_prim, float* out_tuv) {
  if (!c || !rays || !out_prim || !out_tuv || mode < 0 || mode > 2) return BDPT_E_INVALID;
  if (!c->scene.have) return BDPT_E_STATE;
  ENTER(c);
  DevPool pool;
  const float* dr;
  int32_t* dp;
  float* dt;
  int rc;
  if ((rc = devUpload(c, pool, &dr, rays, (size_t)n * 8)) || (rc = devAlloc(c, pool, &dp, n)) ||
      (rc = devAlloc(c, pool, &dt, (size_t)n * 3)))
    return rc;
  launchTestTrace(c->scene.S, dr, n, mode, dp, dt, nullptr);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out_prim, dp, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out_tuv, dt, (size_t)n * 12, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    fail(c, hipGetErrorString(e));
    return BDPT_E_HIP;
  }
  return BDPT_OK;
}

int bdpt_test_trace_shadow(bdpt_ctx* c, const float* rays, uint32_t n, uint8_t* out_vis, uint32_t* out_max_stack) {
  if (!c || !rays || !out_vis || !n) return BDPT_E_INVALID;
  if (!c->scene.have) return BDPT_E_STATE;
  ENTER(c);
  // SoA planes as the ray queue holds them; tmin comes from ray 0 (the kernel takes one tmin per launch)
  std::vector<float> planes((size_t)7 * n);
  for (uint32_t i = 0; i < n; i++) {
    const float* r = rays + (size_t)i * 8;
    for (int k = 0; k < 6; k++) planes[(size_t)k * n + i] = r[k];
    planes[(size_t)6 * n + i] = r[7];
  }
  std::vector<uint32_t> cursors(2 * kCursorStride, 0u);
  cursors[0] = n;  // count; head = cursors[kCursorStride] = 0
  DevPool pool;
  const float* dp;
  const uint32_t* dc;
  uint8_t* dv;
  DevCounters* dcnt;
  int rc;
  if ((rc = devUpload(c, pool, &dp, planes.data(), planes.size())) || (rc = devUpload(c, pool, &dc, cursors.data(), cursors.size())) ||
      (rc = devAlloc(c, pool, &dv, (size_t)n)) || (rc = devAlloc(c, pool, &dcnt, 1)))
    return rc;
  hipError_t e = hipMemset(dcnt, 0, sizeof(DevCounters));
  if (e == hipSuccess) {
    launchTestTraceShadow(c->scene.S, dp, n, dc, const_cast<uint32_t*>(dc) + kCursorStride, dv, dcnt, rays[6], c->numCUs, nullptr);
    e = hipDeviceSynchronize();
  }
  DevCounters h;
  if (e == hipSuccess) e = hipMemcpy(out_vis, dv, (size_t)n, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(&h, dcnt, sizeof(h), hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    fail(c, hipGetErrorString(e));
    return BDPT_E_HIP;
  }
  if (out_max_stack) {
    unsigned long long m = 0;
    for (uint32_t sh = 0; sh < kCounterShards; sh++) m = std::max(m, h.v[sh][C_STACK_MAX]);
    *out_max_stack = (uint32_t)m;
  }
  return BDPT_OK;
}

int bdpt_test_area_light_sample(bdpt_ctx* c, uint32_t mode, const uint32_t* states, const float* points, uint32_t n, float* out) {
  if (!c || !states || !out || mode > 1 || (mode == 1 && !points)) return BDPT_E_INVALID;
  if (!c->scene.have) return refuse(c, BDPT_E_STATE, "test_area_light_sample", "no scene");
  ENTER(c);
  if (int rc = ensureAreaLights(c, nullptr)) return rc;
  if (!n) return BDPT_OK;
  DevPool pool;
  const uint32_t* ds = nullptr;
  const float* dp = nullptr;
  float* dout = nullptr;
  int rc;
  if ((rc = devUpload(c, pool, &ds, states, n)) || (mode == 1 && (rc = devUpload(c, pool, &dp, points, (size_t)n * 3))) ||
      (rc = devAlloc(c, pool, &dout, (size_t)n * 16)))
    return rc;
  hipError_t e = hipDeviceSynchronize();  // (the last update's refresh)
  if (e == hipSuccess) {
    if (c->scene.area.n)
      launchTestAreaSample(c->scene.S, c->scene.area, (int)mode, ds, dp, n, dout, nullptr);
    else
      e = hipMemset(dout, 0, (size_t)n * 64);  // no emitter: every output is zero
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)n * 64, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    fail(c, hipGetErrorString(e));
    return BDPT_E_HIP;
  }
  return BDPT_OK;
}

int bdpt_test_alpha(bdpt_ctx* c, uint32_t variant, const uint32_t* prim, const float* uv, uint32_t n, uint8_t* out_fails) {
  if (!c || !prim || !uv || !out_fails || variant > 2) return BDPT_E_INVALID;
  if (!c->scene.have) return refuse(c, BDPT_E_STATE, "test_alpha", "no scene");
  ENTER(c);
  for (uint32_t i = 0; i < n; i++)
    if (prim[i] >= c->scene.numTriangles) return refuse(c, BDPT_E_INVALID, "test_alpha", "a prim is not a triangle of the scene");
  if (!n) return BDPT_OK;
  DevPool pool;
  const uint32_t* dp = nullptr;
  const float* duv = nullptr;
  uint8_t* dout = nullptr;
  int rc;
  if ((rc = devUpload(c, pool, &dp, prim, n)) || (rc = devUpload(c, pool, &duv, uv, (size_t)n * 2)) || (rc = devAlloc(c, pool, &dout, (size_t)n)))
    return rc;
  launchTestAlpha(c->scene.S, c->scene.alphaTris, c->scene.alphaTris ? c->scene.numAlphaTris : 0u, variant, dp, duv, n, dout, nullptr);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out_fails, dout, (size_t)n, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    fail(c, hipGetErrorString(e));
    return BDPT_E_HIP;
  }
  return BDPT_OK;
}

int bdpt_test_bsdf(bdpt_ctx* c, const float* in, uint32_t n, uint32_t matIndex, float* out) {
  if (!c || !in || !out) return BDPT_E_INVALID;
  ENTER(c);
  DevPool pool;
  const float* di;
  float* dout;
  int rc;
  if ((rc = devUpload(c, pool, &di, in, (size_t)n * 20)) || (rc = devAlloc(c, pool, &dout, (size_t)n * 16)))
    return rc;
  launchTestBsdf(di, n, matIndex, dout, nullptr);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)n * 64, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    fail(c, hipGetErrorString(e));
    return BDPT_E_HIP;
  }
  return BDPT_OK;
}

// Test hook: the sampling table of bdpt_env_prepare, read back
int bdpt_test_env_table(bdpt_ctx* c, uint32_t* cdf, uint64_t* rowCdf) {
  if (!c || !cdf || !rowCdf) return BDPT_E_INVALID;
  if (!c->envTable.ready) return refuse(c, BDPT_E_STATE, "test_env_table", "no sampling table (bdpt_env_prepare first)");
  ENTER(c);
  HIPCHK(c, hipDeviceSynchronize());
  const EnvTable& T = c->envTable.table;
  HIPCHK(c, hipMemcpy(cdf, T.cdf, (size_t)T.W * T.H * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(rowCdf, T.rowCdf, (size_t)T.H * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return BDPT_OK;
}

}  // extern "C"
