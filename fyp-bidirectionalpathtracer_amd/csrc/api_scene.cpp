// api_scene.cpp — the scene of the C ABI (include/bdpt.h): bdpt_set_scene (validation, uploads, the BVH build and what
// is derived from them, in named stages), camera and environment, the emitter table of area lights, and the BVH's summary
// and hashes.  bdpt_set_scene, ensureAreaLights' first build and the hashes allocate and synchronise the device: not
// inside a stream capture.  bdpt_set_scene is not transactional: validation refuses with the old scene in place, any
// later failure leaves the context without a scene.  bdpt_set_camera and bdpt_set_environment only store their argument
// (the latter drops the sampling table bdpt_env_prepare made for the old map).
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <new>
#include <string>
#include <vector>

#include "api_common.hpp"
#include "scene_bvh.h"

using namespace bdpt;

namespace {
// The alpha-quad plane of an RGBA8 texture (texture_planes.h alphaQuadRows), rows spread over the host threads
std::vector<uint32_t> alphaQuadPlane(const bdpt_texture& t) {
  std::vector<uint32_t> q((size_t)t.width * t.height);
  hostParallelFor(t.height, [&](size_t y0, size_t y1) { alphaQuadRows(t.rgba8, t.width, t.height, (uint32_t)y0, (uint32_t)y1, q.data()); });
  return q;
}

// The scene's acceleration structure built on `device` (bvh_device.hip: references, binary tree, collapse and packed
// records — the records the host code produces, bit for bit).  The one place that reads the build's measurement knobs,
// at every call: BDPT_HOST_PRIORITIES (the host decides what the clipper leaves, priorities and split counts),
// BDPT_UPLOAD_TRI_RECS (the host's triangle records and boxes are uploaded).
void buildSceneBvhOnDevice(const bdpt_scene_desc* d, int device, bool classify, SceneBvh& sb, std::string& error) {
  struct Build {
    BvhDeviceBuild* b;
    ~Build() { bvhDeviceBuildEnd(b); }
  } build{bvhDeviceBuildBegin(device)};
  BvhBackend be;
  be.user = build.b;
  be.makeRefs = makeReferencesOnDevice;
  be.buildTree = buildBinaryTreeOnDevice;
  be.pack = packOnDevice;
  be.hostPriorities = std::getenv("BDPT_HOST_PRIORITIES") != nullptr;
  be.uploadTriRecs = std::getenv("BDPT_UPLOAD_TRI_RECS") != nullptr;
  buildSceneBvh(d, 0, -1.0f, -1.0f, classify, sb, &be, &error);
}

// ---- bdpt_set_scene, in stages: each is a function of the description and the scene state `s` it fills ----

// What can be refused while the old scene is still in place.
int validateScene(bdpt_ctx* c, const bdpt_scene_desc* d) {
  if (!d->positions || !d->normals || !d->indices || !d->triMaterial || !d->materials || !d->numMaterials) {
    fail(c, "scene: positions, normals, indices, triMaterial and materials are required");
    return BDPT_E_INVALID;
  }
  if (d->numLights == 0 || !d->lights) {
    fail(c, "scene: at least one light is required (SceneLoaderWrapper adds a directional light when a file has none)");
    return BDPT_E_INVALID;
  }
  if (d->numLights > BDPT_MAX_LIGHTS) return refuse(c, BDPT_E_LIMIT, "scene", "more than BDPT_MAX_LIGHTS lights");
  if (d->numTriangles >= (1u << 28)) return refuse(c, BDPT_E_LIMIT, "scene", "triangle count exceeds the 2^28 leaf-reference limit");
  std::atomic<int> bad{0};  // 1 = material id, 2 = vertex index, 3 = vertex position
  hostParallelFor(d->numTriangles, [&](size_t t0, size_t t1) {
    for (size_t t = t0; t < t1; t++) {
      if (d->triMaterial[t] >= d->numMaterials) bad.store(1);
      for (int k = 0; k < 3; k++) {
        const uint32_t vi = d->indices[t * 3 + (size_t)k];
        if (vi >= d->numVertices) {
          bad.store(2);
          continue;
        }
        // (a box with a NaN or an infinity in it has no place in a tree built by comparing and sorting boxes)
        const float* p = d->positions + (size_t)vi * 3;
        if (!(bvhCoordInRange(p[0]) && bvhCoordInRange(p[1]) && bvhCoordInRange(p[2])) && bad.load() == 0) bad.store(3);
      }
    }
  });
  if (bad.load() == 3) return refuse(c, BDPT_E_INVALID, "scene", "a triangle has a vertex position that is not finite or lies beyond 2^60");
  if (bad.load() == 1) return refuse(c, BDPT_E_INVALID, "scene", "triMaterial out of range");
  if (bad.load() == 2) return refuse(c, BDPT_E_INVALID, "scene", "vertex index out of range");
  for (uint32_t m = 0; m < d->numMaterials; m++) {
    const bdpt_material& mm = d->materials[m];
    const int ids[4] = {mm.texBaseColor, mm.texSpecular, mm.texEmissive, mm.texNormal};
    for (int id : ids)
      if (id < -1 || id >= (int)d->numTextures) return refuse(c, BDPT_E_INVALID, "scene", "material texture index out of range");
  }
  return BDPT_OK;
}

// Beside the build, on a thread of its own: the per-primitive shading records (3 x (position, normal, uv) + material id,
// 112 B in a 128-byte slot) and the uploads that depend on nothing the build produces — while the build's device stages run the host is
// idle, and while its host stages run the copy engine is.
struct SideUploads {
  DevPool pool;
  const float* shade = nullptr;
  const uint32_t* indices = nullptr;
  const float* bitangents = nullptr;
  hipError_t err = hipSuccess;
  std::string what;  // the staged upload's own message, when that is what failed
};
SideUploads sideUploads(int device, const bdpt_scene_desc* d) {
  SideUploads u;
  BigVec<float> shade((size_t)d->numTriangles * kShadeRecF4 * 4);  // (sized, not zeroed: the loop writes every float)
  hostParallelFor(d->numTriangles, [&](size_t t0, size_t t1) {
    for (size_t t = t0; t < t1; t++) {
      float* r = &shade[t * kShadeRecF4 * 4];
      for (int k = 0; k < 3; k++) {
        const uint32_t vi = d->indices[t * 3 + (size_t)k];
        const float* p = d->positions + (size_t)vi * 3;
        const float* nn = d->normals + (size_t)vi * 3;
        float* q = r + k * 8;
        q[0] = p[0];
        q[1] = p[1];
        q[2] = p[2];
        q[3] = nn[0];
        q[4] = nn[1];
        q[5] = nn[2];
        q[6] = d->texcoords ? d->texcoords[(size_t)vi * 3] : 0.0f;
        q[7] = d->texcoords ? d->texcoords[(size_t)vi * 3 + 1] : 0.0f;
      }
      uint32_t mid = d->triMaterial[t];
      std::memcpy(r + 24, &mid, 4);
      for (int k = 25; k < kShadeRecF4 * 4; k++) r[k] = 0.0f;
    }
  });
  auto up = [&](auto** dst, const auto* host, size_t count) {
    if (u.err != hipSuccess) return;
    void* q = nullptr;
    u.err = hipMalloc(&q, std::max<size_t>(count * sizeof(**dst), 16));
    if (u.err != hipSuccess) return;
    u.pool.ptrs.push_back(q);
    if (count) {
      std::string e;
      if (!bvhUploadStaged(q, host, count * sizeof(**dst), e)) {
        u.err = hipErrorUnknown;
        u.what = e;
      }
    }
    *dst = static_cast<std::remove_reference_t<decltype(*dst)>>(q);
  };
  u.err = hipSetDevice(device);
  up(&u.shade, shade.data(), shade.size());
  up(&u.indices, d->indices, (size_t)d->numTriangles * 3);
  if (d->bitangents) up(&u.bitangents, d->bitangents, (size_t)d->numVertices * 3);
  return u;
}
// the thread's results become the scene's (a std::bad_alloc of that thread is rethrown here: bdpt_set_scene's catch)
int joinSideUploads(bdpt_ctx* c, const bdpt_scene_desc* d, SceneState& s, std::future<SideUploads>& side) {
  SideUploads u = side.get();
  u.pool.moveTo(s.allocs);
  if (u.err != hipSuccess) {
    fail(c, std::string("scene upload: ") + (u.what.empty() ? std::string(hipGetErrorString(u.err)) : u.what));
    return u.err == hipErrorOutOfMemory ? BDPT_E_NOMEM : BDPT_E_HIP;
  }
  s.S.shade = reinterpret_cast<const float4*>(u.shade);
  s.S.indices = u.indices;
  if (d->bitangents) {
    s.S.bitangents = u.bitangents;
    s.S.hasBitangents = 1;
  }
  return BDPT_OK;
}

// traversal flags, alpha classification, spatial pre-splitting and the tree itself (scene_bvh.cpp); the records and the
// summary become the scene's
int buildTree(bdpt_ctx* c, const bdpt_scene_desc* d, SceneState& s, SceneBvh& sb) {
  try {
    std::string treeError;
    buildSceneBvhOnDevice(d, c->device, std::getenv("BDPT_NO_ALPHA_CLASSIFY") == nullptr, sb, treeError);
    if (sb.bvh.deviceRecs) s.allocs.ptrs.push_back(sb.bvh.deviceRecs);  // (the context's from here on)
    if (!treeError.empty()) {
      fail(c, "scene: " + treeError);
      return treeError.find("2^31") != std::string::npos ? BDPT_E_LIMIT : (treeError.find("out of device memory") != std::string::npos ? BDPT_E_NOMEM : BDPT_E_HIP);
    }
  } catch (const std::bad_alloc&) {
    fail(c, "scene: out of host memory while building the acceleration structure");
    return BDPT_E_NOMEM;
  }
  Bvh& bvh = sb.bvh;
  if (bvh.maxStack > (uint32_t)kBvhMaxStack) {
    fail(c, "bvh needs a deeper traversal stack than the device provides");
    return BDPT_E_LIMIT;
  }
  if (!bvh.deviceRecs && !bvh.recs.empty()) {  // nothing to build a tree over (no triangle can be hit): the host's one empty node
    const BvhRec* dRecs = nullptr;
    if (int rc0 = devUpload(c, s.allocs, &dRecs, bvh.recs.data(), bvh.recs.size())) return rc0;
    bvh.deviceRecs = const_cast<BvhRec*>(dRecs);
    bvh.deviceNumRecs = bvh.recs.size();
  }
  if (!bvh.deviceRecs) return refuse(c, BDPT_E_HIP, "scene", "the acceleration structure has no records");
  s.bvhInfo.numNodes = bvh.numNodes;
  s.bvhInfo.numTriangles = d->numTriangles;
  s.bvhInfo.maxDepth = bvh.maxDepth;
  s.bvhInfo.nodeBytes = sizeof(BvhRec);
  s.bvhInfo.triBytes = sizeof(BvhTri);
  s.bvhInfo.sahCost = bvh.sahCost;
  s.bvhInfo.maxStack = bvh.maxStack;
  s.bvhInfo.numReferences = bvh.numRefs;
  s.bvhInfo.numDropped = bvh.numDropped;
  s.bvhInfo.numAlphaMode = sb.numAlphaMode;
  s.bvhInfo.numAlwaysPass = sb.numAlwaysPass;
  return BDPT_OK;
}

int uploadMaterials(bdpt_ctx* c, const bdpt_scene_desc* d, SceneState& s) {
  int rc;
  if ((rc = devUpload(c, s.allocs, &s.S.materials, d->materials, d->numMaterials))) return rc;
  std::vector<TexDev> texs(d->numTextures);
  for (uint32_t i = 0; i < d->numTextures; i++) {
    const bdpt_texture& t = d->textures[i];
    if (!t.rgba8 || !t.width || !t.height) return refuse(c, BDPT_E_INVALID, "scene", "empty texture");
    // one spare texel after the last: the row-pair load of the last texel (device_scene.hpp texelRow) stays inside
    const size_t bytes = (size_t)t.width * t.height * 4;
    uint8_t* px = nullptr;
    if ((rc = devAlloc(c, s.allocs, &px, bytes + 4))) return rc;
    HIPCHK(c, hipMemset(px + bytes, 0, 4));
    std::string e;
    if (!bvhUploadStaged(px, t.rgba8, bytes, e)) {
      fail(c, e);
      return BDPT_E_HIP;
    }
    texs[i] = TexDev{px, t.width, t.height, t.srgb, texPow2Flags(t.width, t.height)};
  }
  if ((rc = devUpload(c, s.allocs, &s.S.textures, texs.data(), texs.size()))) return rc;
  std::vector<TexDev> matTex((size_t)d->numMaterials * 4, TexDev{nullptr, 0, 0, 0, 0});
  for (uint32_t mi = 0; mi < d->numMaterials; mi++) {
    const bdpt_material& mm = d->materials[mi];
    const int ids[4] = {mm.texBaseColor, mm.texSpecular, mm.texEmissive, mm.texNormal};
    for (int k = 0; k < 4; k++)
      if (ids[k] >= 0) matTex[(size_t)mi * 4 + k] = texs[(size_t)ids[k]];
  }
  return devUpload(c, s.allocs, &s.S.matTex, matTex.data(), matTex.size());
}

// the alpha-test records of the non-opaque triangles, made on the device from the shading records and the material
// tables already there (kernels.hip alpha_recs_kernel): only the list of those triangles crosses the bus
int makeAlphaRecords(bdpt_ctx* c, const bdpt_scene_desc* d, SceneState& s, const std::vector<uint32_t>& alphaTris) {
  int rc;
  float4* dAlpha = nullptr;
  if ((rc = devAlloc(c, s.allocs, &dAlpha, std::max<size_t>(alphaTris.size(), 1) * 4))) return rc;
  if (alphaTris.empty()) {
    HIPCHK(c, hipMemset(dAlpha, 0, 4 * sizeof(float4)));
  } else {
    // an alpha-quad plane for every base-colour texture an alpha test samples (device_scene.hpp alphaQuad): the
    // materials of the listed triangles (the ids their shading records carry), under the record builder's own rule
    // (alphaSamplesTexture), so that every mode-2 record alpha_recs_kernel writes has its plane
    std::vector<uint8_t> alphaMat(d->numMaterials, 0);
    for (const uint32_t t : alphaTris) alphaMat[d->triMaterial[t]] = 1;
    std::vector<unsigned long long> quadByTex(std::max<size_t>(d->numTextures, 1), 0ull);
    for (uint32_t mi = 0; mi < d->numMaterials; mi++) {
      const bdpt_material& mm = d->materials[mi];
      if (!alphaMat[mi] || !alphaSamplesTexture(BDPT_FLAG_DIFFUSE_TYPE(mm.flags), mm.texBaseColor) || quadByTex[(size_t)mm.texBaseColor])
        continue;
      const std::vector<uint32_t> plane = alphaQuadPlane(d->textures[mm.texBaseColor]);
      const uint32_t* dPlane = nullptr;
      if ((rc = devUpload(c, s.allocs, &dPlane, plane.data(), plane.size()))) return rc;
      quadByTex[(size_t)mm.texBaseColor] = (unsigned long long)reinterpret_cast<uintptr_t>(dPlane);
    }
    const uint32_t* dList = nullptr;
    const unsigned long long* dQuad = nullptr;
    DevPool scratch;
    // (the list stays: the emitter table of area lights finds a triangle's alpha-test record in it)
    if ((rc = devUpload(c, s.allocs, &dList, alphaTris.data(), alphaTris.size())) ||
        (rc = devUpload(c, scratch, &dQuad, quadByTex.data(), quadByTex.size())))
      return rc;
    s.alphaTris = dList;
    s.numAlphaTris = (uint32_t)alphaTris.size();
    launchAlphaRecs(s.S, dList, (uint32_t)alphaTris.size(), dQuad, dAlpha, nullptr);
    const hipError_t e = hipDeviceSynchronize();
    HIPCHK(c, e);
  }
  s.S.alphaRecs = dAlpha;
  return BDPT_OK;
}

// The lights and the sRGB table, then the occluder hints of next-event rays: one cube map of nearest triangles per light
// (directional lights: empty), traced here once.
int uploadLights(bdpt_ctx* c, const bdpt_scene_desc* d, SceneState& s) {
  int rc;
  SceneConst sc;
  std::memset(&sc, 0, sizeof(sc));
  std::memcpy(sc.lights, d->lights, sizeof(bdpt_light) * d->numLights);
  for (int i = 0; i < 256; i++) {
    double cc = (double)i / 255.0;
    double l = (cc <= 0.04045) ? cc / 12.92 : std::pow((cc + 0.055) / 1.055, 2.4);
    sc.srgbLut[i] = (float)l;
  }
  if ((rc = devUpload(c, s.allocs, &s.S.sc, &sc, 1))) return rc;
  s.S.numLights = d->numLights;
  s.hints = std::getenv("BDPT_NO_HINTS") == nullptr;
  if (!s.hints) return BDPT_OK;
  uint32_t res = 512;
  if (const char* e = std::getenv("BDPT_LIGHT_MAP_RES")) res = (uint32_t)std::max(0, std::min(2048, std::atoi(e)));
  if (!res) return BDPT_OK;
  uint32_t* maps = nullptr;
  if ((rc = devAlloc(c, s.allocs, &maps, (size_t)6 * res * res * d->numLights))) return rc;
  launchLightMaps(s.S, maps, res, nullptr);
  HIPCHK(c, hipDeviceSynchronize());
  s.S.lightMap = maps;
  s.S.lightMapRes = res;
  s.lightMaps = maps;
  return BDPT_OK;
}

// Not transactional: once validation has passed the old scene is gone, whatever happens after.
int setSceneImpl(bdpt_ctx* c, const bdpt_scene_desc* d) {
  if (!c || !d) return BDPT_E_INVALID;
  if (int rc = validateScene(c, d)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  dropScene(c);
  SceneState& s = c->scene;

  // BDPT_BUILD_VERBOSE: where the set-up time goes (stderr), as bvh_build.cpp's own laps
  const bool verbose = std::getenv("BDPT_BUILD_VERBOSE") != nullptr;
  auto tLap = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (!verbose) return;
    const auto t = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[set_scene] %-18s %.3f s\n", what, std::chrono::duration<double>(t - tLap).count());
    tLap = t;
  };
  lap("validate");
  // (BDPT_SET_SCENE_SERIAL: measurement knob — the same work at the point where its results are needed, on this thread)
  std::future<SideUploads> side =
      std::async(std::getenv("BDPT_SET_SCENE_SERIAL") ? std::launch::deferred : std::launch::async, sideUploads, c->device, d);
  struct SideJoin {  // whatever way this function is left, the thread is joined (and what it allocated goes with its pool)
    std::future<SideUploads>& f;
    ~SideJoin() {
      if (!f.valid()) return;
      try {
        f.get();
      } catch (...) {
      }
    }
  } sideJoin{side};
  int rc;
  SceneBvh sb;
  if ((rc = buildTree(c, d, s, sb))) return rc;
  lap("buildSceneBvh");
  if ((rc = joinSideUploads(c, d, s, side))) return rc;
  lap("shading records + uploads (joined)");
  s.S.recs = reinterpret_cast<const uint4*>(sb.bvh.deviceRecs);
  s.S.numRecs = (uint32_t)sb.bvh.deviceNumRecs;
  if ((rc = uploadMaterials(c, d, s)) || (rc = makeAlphaRecords(c, d, s, sb.alphaTris))) return rc;
  lap("indices, textures, alpha");
  if ((rc = uploadLights(c, d, s))) return rc;
  // the primary-visibility hints of an earlier scene index records that are gone
  if (c->frame.hintPix) HIPCHK(c, hipMemset(c->frame.hintPix, 0xFF, (size_t)c->frame.W * c->frame.H * sizeof(uint32_t)));
  c->frame.hintCamValid = false;
  lap("light maps");
  s.numVertices = d->numVertices;
  s.numTriangles = d->numTriangles;
  s.have = true;
  return BDPT_OK;
}
}  // namespace

// (declared in api_common.hpp)  Triangles the build dropped (alpha clipping) are found through the
// refit plan's leaves, which is made for that when the scene has any.
int bdpt::ensureAreaLights(bdpt_ctx* c, hipStream_t st) {
  if (c->scene.areaReady) return BDPT_OK;
  if (streamIsCapturing(st)) {
    fail(c, "area lights: the emitter table needs bdpt_prepare(BDPT_PREPARE_AREA_LIGHTS) before stream capture");
    return BDPT_E_STATE;
  }
  HIPCHK(c, hipDeviceSynchronize());
  const uint32_t nt = c->scene.numTriangles;
  const size_t nb = wavesFor(nt);
  DevPool scratch;
  uint8_t* referenced = nullptr;
  int rc;
  if (c->scene.bvhInfo.numDropped) {
    if ((rc = ensureRefit(c, st))) return rc;
    if ((rc = devAlloc(c, scratch, &referenced, nt))) return rc;
    HIPCHK(c, hipMemset(referenced, 0, nt));
    launchAreaMarkReferenced(c->scene.refit.nodes, c->scene.refit.numNodes, c->scene.S.recs, referenced, nullptr);
  }
  uint32_t *blockCount = nullptr, *blockBase = nullptr, *counts = nullptr;
  if ((rc = devAlloc(c, scratch, &blockCount, nb)) || (rc = devAlloc(c, scratch, &blockBase, nb)) || (rc = devAlloc(c, scratch, &counts, 2)))
    return rc;
  HIPCHK(c, hipMemset(counts, 0, 2 * sizeof(uint32_t)));
  launchAreaCount(c->scene.S, nt, referenced, blockCount, blockBase, counts, nullptr);
  uint32_t hc[2] = {0, 0};
  HIPCHK(c, hipMemcpy(hc, counts, sizeof(hc), hipMemcpyDeviceToHost));
  AreaDev A{};
  A.n = hc[0];
  if (A.n) {
    const size_t nbe = wavesFor(A.n);
    float *cdf = nullptr, *total = nullptr;
    float4* emit = nullptr;
    if ((rc = devAlloc(c, c->scene.allocs, &cdf, A.n)) || (rc = devAlloc(c, c->scene.allocs, &emit, A.n)) ||
        (rc = devAlloc(c, c->scene.allocs, &total, 2)) || (rc = devAlloc(c, c->scene.allocs, &c->scene.areaBlockSum, nbe)) ||
        (rc = devAlloc(c, c->scene.allocs, &c->scene.areaBlockLast, nbe)))
      return rc;
    A.cdf = cdf;
    A.emit = emit;
    A.total = total;
    launchAreaCompact(c->scene.S, nt, referenced, blockBase, c->scene.alphaTris, c->scene.numAlphaTris, emit, nullptr);
    launchAreaRefresh(c->scene.S, A, c->scene.areaBlockSum, c->scene.areaBlockLast, nullptr);
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipDeviceSynchronize());
  c->scene.area = A;
  c->scene.areaTextured = hc[1];
  c->scene.areaReady = true;
  return BDPT_OK;
}

extern "C" {

// Nothing thrown while the scene is copied and its acceleration structure built — on this thread or on a builder
// worker (bvh.h WorkerScope) — crosses the C boundary: the large allocations of a 10 M-triangle scene fail as BDPT_E_NOMEM.
int bdpt_set_scene(bdpt_ctx* c, const bdpt_scene_desc* d) {
  try {
    return setSceneImpl(c, d);
  } catch (const std::bad_alloc&) {
    fail(c, "scene: out of host memory while building the acceleration structure");
    return BDPT_E_NOMEM;
  } catch (const std::exception& e) {
    fail(c, std::string("scene: ") + e.what());
    return BDPT_E_INVALID;
  }
}

int bdpt_get_bvh_info(const bdpt_ctx* c, bdpt_bvh_info* out) {
  if (!c || !out) return BDPT_E_INVALID;
  if (!c->scene.have) return BDPT_E_STATE;
  *out = c->scene.bvhInfo;
  return BDPT_OK;
}

int bdpt_set_camera(bdpt_ctx* c, const bdpt_camera* cam) {
  if (!c || !cam) return BDPT_E_INVALID;
  c->cam = *cam;
  c->haveCamera = true;
  return BDPT_OK;
}

int bdpt_set_environment(bdpt_ctx* c, const bdpt_environment* env) {
  if (!c) return BDPT_E_INVALID;
  if (env && env->envMap && (!env->width || !env->height)) return refuse(c, BDPT_E_INVALID, "environment", "a map needs a width and a height");
  if (!c->envTable.allocs.ptrs.empty()) {  // a sampling table made for the old map goes with it (it may still be read)
    ENTER(c);
    HIPCHK(c, hipDeviceSynchronize());
  }
  dropEnv(c->envTable);
  c->env = env ? *env : bdpt_environment{};
  if (!c->env.envMap) c->env.width = c->env.height = 0;
  return BDPT_OK;
}

// The sampling table of the bound map (env_light.hip): allocated on first use or when the size changes (not while
// capturing), rebuilt by three stream-ordered launches on every call.
int bdpt_env_prepare(bdpt_ctx* c, void* stream) {
  if (!c) return BDPT_E_INVALID;
  if (!c->env.envMap) return refuse(c, BDPT_E_STATE, "env_prepare", "no environment map (bdpt_set_environment with a map first)");
  const uint32_t W = c->env.width, H = c->env.height;
  if (W > kEnvMaxDim || H > kEnvMaxDim) return refuse(c, BDPT_E_LIMIT, "env_prepare", "the map exceeds BDPT_ENV_MAX_DIM in width or height");
  if (!aligned(c->env.envMap, 16)) return refuse(c, BDPT_E_INVALID, "env_prepare", "the map must be 16-byte aligned");
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  EnvState& E = c->envTable;
  if (E.allocs.ptrs.empty() || E.table.W != W || E.table.H != H) {
    if (streamIsCapturing(st)) return refuse(c, BDPT_E_STATE, "env_prepare", "the first call for a map size allocates: not inside a stream capture");
    HIPCHK(c, hipDeviceSynchronize());
    dropEnv(E);
    EnvState fresh;
    uint32_t* cdf = nullptr;
    uint64_t* rowCdf = nullptr;
    int rc;
    if ((rc = devAlloc(c, fresh.allocs, &cdf, (size_t)W * H)) || (rc = devAlloc(c, fresh.allocs, &rowCdf, (size_t)H)) ||
        (rc = devAlloc(c, fresh.allocs, &fresh.maxBits, (size_t)4)))
      return rc;
    HIPCHK(c, hipMemset(fresh.maxBits, 0, 16));
    fresh.table = EnvTable{c->env.envMap, W, H, cdf, rowCdf};
    fresh.bytes = (uint64_t)W * H * sizeof(uint32_t) + (uint64_t)H * sizeof(uint64_t) + 16;
    E = std::move(fresh);
  }
  E.table.map = c->env.envMap;
  if (int rc = orderAfterLast(c, st)) return rc;
  E.ready = false;
  launchEnvTable(E.table.map, W, H, const_cast<uint32_t*>(E.table.cdf), const_cast<uint64_t*>(E.table.rowCdf), E.maxBits, st);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) {
    // a launch that failed midway may have left the maximum's word non-zero: the table goes, the next call builds afresh
    fail(c, std::string("env_prepare: ") + hipGetErrorString(e));
    (void)hipDeviceSynchronize();
    dropEnv(E);
    return BDPT_E_HIP;
  }
  c->lastStream = st;
  E.ready = true;
  return BDPT_OK;
}

int bdpt_get_env_info(bdpt_ctx* c, bdpt_env_info* out) {
  if (!c || !out) return BDPT_E_INVALID;
  if (!c->envTable.ready) return refuse(c, BDPT_E_STATE, "get_env_info", "no sampling table (bdpt_env_prepare first)");
  ENTER(c);
  HIPCHK(c, hipDeviceSynchronize());
  const EnvState& E = c->envTable;
  *out = bdpt_env_info{};
  out->width = E.table.W;
  out->height = E.table.H;
  uint32_t bits = 0;
  HIPCHK(c, hipMemcpy(&out->total, E.table.rowCdf + (E.table.H - 1), sizeof(uint64_t), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(&bits, E.maxBits + 1, sizeof(bits), hipMemcpyDeviceToHost));
  std::memcpy(&out->max, &bits, sizeof(bits));
  out->rowScanChunk = kEnvRowScanChunk;
  out->marginalChunk = kEnvMarginalChunk;
  out->tableBytes = E.bytes;
  out->cdf = E.table.cdf;
  out->rowCdf = E.table.rowCdf;
  return BDPT_OK;
}

// Test hook: FNV-1a over the context's records as they stand (synchronises)
int bdpt_ctx_recs_hash(bdpt_ctx* c, uint64_t* out_hash) {
  if (!c || !out_hash) return BDPT_E_INVALID;
  if (!c->scene.have) return BDPT_E_STATE;
  ENTER(c);
  HIPCHK(c, hipDeviceSynchronize());
  std::vector<BvhRec> recs(c->scene.S.numRecs);
  HIPCHK(c, hipMemcpy(recs.data(), c->scene.S.recs, recs.size() * sizeof(BvhRec), hipMemcpyDeviceToHost));
  uint64_t h = 1469598103934665603ull;
  const uint8_t* b = reinterpret_cast<const uint8_t*>(recs.data());
  for (size_t i = 0; i < recs.size() * sizeof(BvhRec); i++) h = (h ^ b[i]) * 1099511628211ull;
  *out_hash = h;
  return BDPT_OK;
}

// Test hook: FNV-1a over the packed records (every node, every leaf triangle, the pad) and the summary of the
// acceleration structure of a scene — device < 0: built, quantised and packed by the host code; device >= 0: as
// bdpt_set_scene does it, tree + quantisation + packing on that device, the records read back.
int bdpt_bvh_recs_hash(const bdpt_scene_desc* d, int device, uint64_t* out_hash, bdpt_bvh_info* out_info) try {
  if (!d || !out_hash || !d->positions || !d->indices || !d->materials || !d->triMaterial || !d->numMaterials) return BDPT_E_INVALID;
  SceneBvh sb;
  BigVec<BvhRec> fromDevice;
  const BvhRec* recs = nullptr;
  size_t numRecs = 0;
  if (device < 0) {
    buildSceneBvh(d, 0, -1.0f, -1.0f, true, sb);
    recs = sb.bvh.recs.data();
    numRecs = sb.bvh.recs.size();
  } else {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device >= count) return BDPT_E_HIP;
    std::string error;
    buildSceneBvhOnDevice(d, device, true, sb, error);
    if (!sb.bvh.deviceRecs && !sb.bvh.recs.empty() && error.empty()) {  // (nothing to build a tree over: the host's one empty node)
      recs = sb.bvh.recs.data();
      numRecs = sb.bvh.recs.size();
    } else {
    if (!sb.bvh.deviceRecs) return BDPT_E_HIP;
    fromDevice.resize(sb.bvh.deviceNumRecs);
    const hipError_t e = hipMemcpy(fromDevice.data(), sb.bvh.deviceRecs, fromDevice.size() * sizeof(BvhRec), hipMemcpyDeviceToHost);
    (void)hipFree(sb.bvh.deviceRecs);
    if (e != hipSuccess || !error.empty()) return BDPT_E_HIP;
    recs = fromDevice.data();
    numRecs = fromDevice.size();
    }
  }
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
  };
  mix(recs, numRecs * sizeof(BvhRec));
  mix(&sb.bvh.maxDepth, sizeof(sb.bvh.maxDepth));
  mix(&sb.bvh.maxStack, sizeof(sb.bvh.maxStack));
  mix(&sb.bvh.sahCost, sizeof(sb.bvh.sahCost));
  *out_hash = h;
  if (out_info) {
    *out_info = bdpt_bvh_info{};
    out_info->numNodes = sb.bvh.numNodes;
    out_info->numTriangles = d->numTriangles;
    out_info->maxDepth = sb.bvh.maxDepth;
    out_info->nodeBytes = sizeof(BvhRec);
    out_info->triBytes = sizeof(BvhTri);
    out_info->sahCost = sb.bvh.sahCost;
    out_info->maxStack = sb.bvh.maxStack;
    out_info->reserved = (uint32_t)numRecs;
    out_info->numReferences = sb.bvh.numRefs;
    out_info->numDropped = sb.bvh.numDropped;
    out_info->numAlphaMode = sb.numAlphaMode;
    out_info->numAlwaysPass = sb.numAlwaysPass;
  }
  return BDPT_OK;
} catch (const std::bad_alloc&) {
  return BDPT_E_NOMEM;
} catch (...) {
  return BDPT_E_INVALID;
}

int bdpt_get_area_light_info(bdpt_ctx* c, bdpt_area_light_info* out) {
  if (!c || !out) return BDPT_E_INVALID;
  if (int rc = needScene(c, "area_light_info")) return rc;
  ENTER(c);
  if (int rc = ensureAreaLights(c, nullptr)) return rc;
  HIPCHK(c, hipDeviceSynchronize());  // (the last update's refresh)
  *out = bdpt_area_light_info{};
  out->numEmitters = c->scene.area.n;
  out->numTextured = c->scene.areaTextured;
  if (c->scene.area.n) HIPCHK(c, hipMemcpy(&out->totalWeight, c->scene.area.total, sizeof(float), hipMemcpyDeviceToHost));
  return BDPT_OK;
}

}  // extern "C"
