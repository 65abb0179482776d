// api.cpp — the C ABI of include/bdpt.h but its per-item queries (api_query.cpp): context, scene upload + BVH build,
// per-tile path buffers, stage launches.  Workspaces are sized by bdpt_set_scene / bdpt_resize / bdpt_prepare, so
// bdpt_gbuffer_execute, bdpt_execute and bdpt_bmfr_execute neither allocate nor synchronise and can be
// captured into a hipGraph.  The one exception is spelled out in bdpt.h: bdpt_execute(in = NULL) and
// bdpt_bmfr_execute allocate their optional buffers on first use when bdpt_prepare was not called, and
// refuse (BDPT_E_STATE) to do so while the stream is being captured.
// Every entry point that launches or allocates makes the context's device current first, so one host
// thread may drive contexts on several GPUs; per-context launch state (persistent grid sizes, counters
// read-back) lives in bdpt_ctx, never in statics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <functional>
#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include <new>

#include "context.hpp"
#include "launch.hpp"
#include "scene_bvh.h"

using namespace bdpt;

namespace {
// path-queue counters, their fetch cursors, then the shadow sub-queue counters and cursors
// (every cursor is sharded: kNumSubQueues words, each on its own 128-byte line — atomics to one line serialise)
constexpr size_t kCountBlocks = 1;  // lengths of the valid-pixel lists
constexpr size_t kHeadBlocks = 2;   // fetch cursors of the walk kernel: pixel list x {eye, light}
constexpr size_t kLazyBlocks = kMaxLazyRounds + 2;
// bdpt_execute_masked's eye list borrows two things no stage before the lazy rounds uses: its items live in the second
// lazy-round list (PathBuf::queue[2], which the first lazy round is the first to write, after the generators that read
// the eye list), its lengths in the last lazy cursor block (rounds use blocks 0 .. kMaxLazyRounds), which the frame's
// clear of kCursorWords zeroes with everything else.  So a masked frame allocates nothing and adds no memset.
constexpr size_t kEyeCountBlock = kLazyBlocks - 1;
static_assert(kEyeCountBlock > (size_t)kMaxLazyRounds, "the eye list's cursor block must be one no lazy round uses");
constexpr size_t kCursorWords = (kCountBlocks + kHeadBlocks + kLazyBlocks) * kCursorBlock + 4 * kRayCursorBlock;  // + ray count / head blocks of two classes
}

namespace {

// [0, n) in contiguous chunks over the builder's host threads (bvhBuildThreads)
template <class F>
void hostParallelFor(size_t n, const F& f) {
  const int threads = bvhBuildThreads();
  if (threads <= 1 || n < 65536) {
    f((size_t)0, n);
    return;
  }
  WorkerScope pool;
  const size_t chunk = (n + (size_t)threads - 1) / (size_t)threads;
  for (int t = 1; t < threads; t++) {
    const size_t a = std::min(n, chunk * (size_t)t), b = std::min(n, a + chunk);
    if (a < b) pool.spawn([&f, a, b] { f(a, b); });
  }
  f((size_t)0, std::min(n, chunk));
  pool.join();
}

// The alpha-quad plane of an RGBA8 texture (texture_planes.h alphaQuadRows), rows spread over the host threads
std::vector<uint32_t> alphaQuadPlane(const bdpt_texture& t) {
  std::vector<uint32_t> q((size_t)t.width * t.height);
  hostParallelFor(t.height, [&](size_t y0, size_t y1) { alphaQuadRows(t.rgba8, t.width, t.height, (uint32_t)y0, (uint32_t)y1, q.data()); });
  return q;
}

template <class T>
int devAlloc(bdpt_ctx* c, std::vector<void*>& pool, T** out, size_t count) {
  void* p = nullptr;
  size_t bytes = std::max<size_t>(count * sizeof(T), 16);
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) {
    fail(c, std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
    return BDPT_E_NOMEM;
  }
  pool.push_back(p);
  *out = reinterpret_cast<T*>(p);
  return BDPT_OK;
}
template <class T>
int devUpload(bdpt_ctx* c, std::vector<void*>& pool, const T** out, const T* host, size_t count) {
  T* d = nullptr;
  int rc = devAlloc(c, pool, &d, count);
  if (rc) return rc;
  if (count) {  // (large arrays through pinned staging: bvhUploadStaged)
    std::string e;
    if (!bvhUploadStaged(d, host, count * sizeof(T), e)) {
      fail(c, e);
      return BDPT_E_HIP;
    }
  }
  *out = d;
  return BDPT_OK;
}
void freePool(std::vector<void*>& pool) {
  for (void* p : pool) (void)hipFree(p);
  pool.clear();
}
// (the device is idle, or the caller has synchronised it)
void dropMorph(bdpt_ctx* c) {
  freePool(c->morphAllocs);
  c->haveMorph = false;
  c->morph = MorphDev{};
  c->morphWeights = nullptr;
}
// (the device is idle, or the caller has synchronised it)
void freeLightGroups(bdpt_ctx* c) {
  if (c->groupSplat) (void)hipFree(c->groupSplat);
  if (c->groupLightIdx) (void)hipFree(c->groupLightIdx);
  c->groupSplat = nullptr;
  c->groupSplatPlanes = 0;
  c->groupLightIdx = nullptr;
}

bool streamIsCapturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) return false;
  return cs != hipStreamCaptureStatusNone;
}

// the six channels of the built-in primary stage; all or nothing
int allocOwnGbuffer(bdpt_ctx* c) {
  if (c->ownGb.worldPosition) return BDPT_OK;
  const size_t n = (size_t)c->W * c->H;
  const size_t mark = c->frameAllocs.size();
  bdpt_gbuffer g{};
  int rc;
  if ((rc = devAlloc(c, c->frameAllocs, &g.worldPosition, n * 4)) || (rc = devAlloc(c, c->frameAllocs, &g.worldNormal, n * 4)) ||
      (rc = devAlloc(c, c->frameAllocs, &g.materialDiffuse, n * 4)) || (rc = devAlloc(c, c->frameAllocs, &g.materialSpecRough, n * 4)) ||
      (rc = devAlloc(c, c->frameAllocs, &g.materialExtraParams, n * 4)) || (rc = devAlloc(c, c->frameAllocs, &g.emissive, n * 4))) {
    while (c->frameAllocs.size() > mark) {
      (void)hipFree(c->frameAllocs.back());
      c->frameAllocs.pop_back();
    }
    return rc;
  }
  c->ownGb = g;
  return BDPT_OK;
}

// ---- the denoiser's history (context.hpp BmfrHistory) ----
// the calls that allocate one ahead of a stream capture, as the refusal inside a capture names them
constexpr const char* kBmfrPrepare = "bdpt_prepare(BDPT_PREPARE_BMFR)";
constexpr const char* kBmfrPlanesPrepare = "bdpt_bmfr_planes_prepare";
// (the device is idle, or the caller has synchronised it)
void freeBmfrHistory(BmfrHistory& h) {
  for (void* p : {(void*)h.pos[0], (void*)h.pos[1], (void*)h.norm[0], (void*)h.norm[1], (void*)h.noisy, (void*)h.filtered, (void*)h.accept,
                  (void*)h.prevPixel})
    if (p) (void)hipFree(p);
  h = BmfrHistory{};
}

int resetBmfrHistory(bdpt_ctx* c, BmfrHistory& h) {
  if (!h.accept) return BDPT_OK;  // nothing allocated yet
  ENTER(c);
  const size_t n = (size_t)c->W * c->H;
  for (int k = 0; k < 2; k++) {
    HIPCHK(c, hipMemset(h.pos[k], 0, n * sizeof(float4)));
    HIPCHK(c, hipMemset(h.norm[k], 0, n * sizeof(float4)));
  }
  HIPCHK(c, hipMemset(h.noisy, 0, 2 * n * sizeof(float4) * h.slots));
  HIPCHK(c, hipMemset(h.filtered, 0, 2 * n * sizeof(float4) * h.slots));
  HIPCHK(c, hipMemset(h.accept, 0, n));
  HIPCHK(c, hipMemset(h.prevPixel, 0, n * sizeof(uint32_t)));
  h.read = 0;
  return BDPT_OK;
}

// History for at least `slots` images.  (Re)allocating resets; replacing a smaller history waits for the device first
// (frames in flight still use it), the first allocation frees nothing and does not wait.  Not while `st` is being
// captured: the message names `who` and the call (`prepare`) that allocates ahead of the capture.
int ensureBmfrHistory(bdpt_ctx* c, BmfrHistory& h, uint32_t slots, hipStream_t st, const char* who, const char* prepare) {
  if (h.accept && h.slots >= slots) return BDPT_OK;
  if (streamIsCapturing(st)) {
    fail(c, std::string(who) + ": the history needs " + prepare + " before stream capture");
    return BDPT_E_STATE;
  }
  if (h.accept) {
    HIPCHK(c, hipDeviceSynchronize());
    freeBmfrHistory(h);
  }
  const size_t n = std::max<size_t>((size_t)c->W * c->H, 1);
  void* a[8]{};
  const size_t bytes[8] = {n * sizeof(float4), n * sizeof(float4), n * sizeof(float4), n * sizeof(float4),
                           2 * n * sizeof(float4) * slots, 2 * n * sizeof(float4) * slots, std::max<size_t>(n, 16), n * sizeof(uint32_t)};
  for (int k = 0; k < 8; k++)
    if (hipMalloc(&a[k], bytes[k]) != hipSuccess) {
      for (int j = 0; j < k; j++) (void)hipFree(a[j]);
      fail(c, std::string(who) + ": hipMalloc of the history failed");
      return BDPT_E_NOMEM;
    }
  h.pos[0] = static_cast<float4*>(a[0]);
  h.pos[1] = static_cast<float4*>(a[1]);
  h.norm[0] = static_cast<float4*>(a[2]);
  h.norm[1] = static_cast<float4*>(a[3]);
  h.noisy = static_cast<float4*>(a[4]);
  h.filtered = static_cast<float4*>(a[5]);
  h.accept = static_cast<uint8_t*>(a[6]);
  h.prevPixel = static_cast<uint32_t*>(a[7]);
  h.slots = slots;
  return resetBmfrHistory(c, h);
}

void stageMark(bdpt_ctx* c, hipStream_t st, const char* name) {
  if (!c->timing || c->numStages >= kMaxStages) return;
  c->stageNames[c->numStages] = name;
  c->numStages++;
  (void)hipEventRecord(c->ev[c->numStages], st);
}
// bracket of a kernel on the second stream: sideBegin before its launch, sideEnd after
void sideBegin(bdpt_ctx* c, hipStream_t side, const char* name) {
  if (!c->timing || c->numSideStages >= bdpt_ctx::kMaxSideStages) return;
  c->sideNames[c->numSideStages] = name;
  (void)hipEventRecord(c->sideEv[2 * c->numSideStages], side);
}
void sideEnd(bdpt_ctx* c, hipStream_t side) {
  if (!c->timing || c->numSideStages >= bdpt_ctx::kMaxSideStages) return;
  (void)hipEventRecord(c->sideEv[2 * c->numSideStages + 1], side);
  c->numSideStages++;
}

// refit (refit.hip, bvh.h "refit"): the plan (a top-down pass over the records, read back once) and the refit's scratch;
// not while capturing
int ensureRefit(bdpt_ctx* c, hipStream_t st) {
  if (c->refitReady) return BDPT_OK;
  if (streamIsCapturing(st)) {
    fail(c, "update: the first update needs bdpt_prepare(BDPT_PREPARE_REFIT) before stream capture");
    return BDPT_E_STATE;
  }
  HIPCHK(c, hipDeviceSynchronize());
  BvhRefitPlan plan;
  {
    std::vector<BvhRec> recs(c->S.numRecs);
    HIPCHK(c, hipMemcpy(recs.data(), c->S.recs, recs.size() * sizeof(BvhRec), hipMemcpyDeviceToHost));
    std::string err;
    if (!bvhRefitMakePlan(recs.data(), recs.size(), plan, err)) {
      fail(c, err);
      return BDPT_E_HIP;
    }
  }
  const size_t nn = std::max<size_t>(plan.nodes.size(), 1);
  RefitDev R{};
  const BvhRefitNode* dNodes = nullptr;
  const uint32_t* dOrder = nullptr;
  int rc;
  if ((rc = devUpload(c, c->sceneAllocs, &dNodes, plan.nodes.data(), plan.nodes.size())) ||
      (rc = devUpload(c, c->sceneAllocs, &dOrder, plan.levelOrder.data(), plan.levelOrder.size())) ||
      (rc = devAlloc(c, c->sceneAllocs, &R.box, nn * 6)) || (rc = devAlloc(c, c->sceneAllocs, &R.childArea, nn * 4)) ||
      (rc = devAlloc(c, c->sceneAllocs, &R.partial, (size_t)kRefitPartials * 6)) || (rc = devAlloc(c, c->sceneAllocs, &R.pad, 1)))
    return rc;
  R.nodes = dNodes;
  R.levelOrder = dOrder;
  R.levelStart = plan.levelStart;
  R.numNodes = (uint32_t)plan.nodes.size();
  c->refit = std::move(R);
  c->refitPlan = std::move(plan);
  c->refitReady = true;
  return BDPT_OK;
}

// bdpt_prepare(BDPT_PREPARE_REFIT_PIECES): the plan as above, then the regions of the tree AS BUILT (bvh.h "piece-tight
// refit", refit.hip k_refit_regions); from then on launchRefit runs its piece-tight instance
int ensureRefitPieces(bdpt_ctx* c) {
  if (c->refitReady && c->refit.region) return BDPT_OK;
  if (c->numUpdates) {
    fail(c, "prepare: BDPT_PREPARE_REFIT_PIECES derives the regions from the tree as built: not after an update (bdpt_set_scene first)");
    return BDPT_E_STATE;
  }
  if (streamIsCapturing(c->lastStream)) {
    fail(c, "prepare: BDPT_PREPARE_REFIT_PIECES allocates and synchronises: not inside a stream capture");
    return BDPT_E_STATE;
  }
  if (int rc = ensureRefit(c, nullptr)) return rc;
  float* region = nullptr;
  if (int rc = devAlloc(c, c->sceneAllocs, &region, (size_t)c->S.numRecs * kPieceFloats)) return rc;
  HIPCHK(c, hipDeviceSynchronize());
  launchRefitRegions(c->refit, reinterpret_cast<const BvhRec*>(c->S.recs), region, nullptr);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipDeviceSynchronize());
  c->refit.region = region;
  return BDPT_OK;
}

}  // namespace

// (declared in context.hpp)
int bdpt::orderAfterLast(bdpt_ctx* c, hipStream_t st) {
  if (c->lastStream != st) {
    HIPCHK(c, hipEventRecord(c->evOrder, c->lastStream));
    HIPCHK(c, hipStreamWaitEvent(st, c->evOrder, 0));
  }
  return BDPT_OK;
}

// (declared in context.hpp)  Triangles the build dropped (alpha clipping) are found through the
// refit plan's leaves, which is made for that when the scene has any.
int bdpt::ensureAreaLights(bdpt_ctx* c, hipStream_t st) {
  if (c->areaReady) return BDPT_OK;
  if (streamIsCapturing(st)) {
    fail(c, "area lights: the emitter table needs bdpt_prepare(BDPT_PREPARE_AREA_LIGHTS) before stream capture");
    return BDPT_E_STATE;
  }
  HIPCHK(c, hipDeviceSynchronize());
  const uint32_t nt = c->numTriangles;
  const size_t nb = wavesFor(nt);
  std::vector<void*> scratch;
  struct Free {
    std::vector<void*>& p;
    ~Free() { freePool(p); }
  } freeScratch{scratch};
  uint8_t* referenced = nullptr;
  int rc;
  if (c->bvhInfo.numDropped) {
    if ((rc = ensureRefit(c, st))) return rc;
    if ((rc = devAlloc(c, scratch, &referenced, nt))) return rc;
    HIPCHK(c, hipMemset(referenced, 0, nt));
    launchAreaMarkReferenced(c->refit.nodes, c->refit.numNodes, c->S.recs, referenced, nullptr);
  }
  uint32_t *blockCount = nullptr, *blockBase = nullptr, *counts = nullptr;
  if ((rc = devAlloc(c, scratch, &blockCount, nb)) || (rc = devAlloc(c, scratch, &blockBase, nb)) || (rc = devAlloc(c, scratch, &counts, 2)))
    return rc;
  HIPCHK(c, hipMemset(counts, 0, 2 * sizeof(uint32_t)));
  launchAreaCount(c->S, nt, referenced, blockCount, blockBase, counts, nullptr);
  uint32_t hc[2] = {0, 0};
  HIPCHK(c, hipMemcpy(hc, counts, sizeof(hc), hipMemcpyDeviceToHost));
  AreaDev A{};
  A.n = hc[0];
  if (A.n) {
    const size_t nbe = wavesFor(A.n);
    float *cdf = nullptr, *total = nullptr;
    float4* emit = nullptr;
    if ((rc = devAlloc(c, c->sceneAllocs, &cdf, A.n)) || (rc = devAlloc(c, c->sceneAllocs, &emit, A.n)) ||
        (rc = devAlloc(c, c->sceneAllocs, &total, 2)) || (rc = devAlloc(c, c->sceneAllocs, &c->areaBlockSum, nbe)) ||
        (rc = devAlloc(c, c->sceneAllocs, &c->areaBlockLast, nbe)))
      return rc;
    A.cdf = cdf;
    A.emit = emit;
    A.total = total;
    launchAreaCompact(c->S, nt, referenced, blockBase, c->alphaTris, c->numAlphaTris, emit, nullptr);
    launchAreaRefresh(c->S, A, c->areaBlockSum, c->areaBlockLast, nullptr);
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipDeviceSynchronize());
  c->area = A;
  c->areaTextured = hc[1];
  c->areaReady = true;
  return BDPT_OK;
}

extern "C" {

int bdpt_create(int device_ordinal, bdpt_ctx** out_ctx) {
  if (!out_ctx) return BDPT_E_INVALID;
  *out_ctx = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_ordinal < 0 || device_ordinal >= n) return BDPT_E_HIP;
  if (hipSetDevice(device_ordinal) != hipSuccess) return BDPT_E_HIP;
  bdpt_ctx* c = new bdpt_ctx();
  c->device = device_ordinal;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_ordinal) == hipSuccess && prop.multiProcessorCount > 0)
    c->numCUs = prop.multiProcessorCount;
  if (hipStreamCreateWithFlags(&c->walkStream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&c->evFork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->evJoin, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->evSplat, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->evStage, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->evOrder, hipEventDisableTiming) != hipSuccess) {
    bdpt_destroy(c);
    return BDPT_E_HIP;
  }
  // traversal-stack overflow rows for the largest persistent grid (kMaxPersistentPerCU waves per CU)
  c->stackOvfStride = (uint32_t)c->numCUs * kMaxPersistentPerCU * kWave;
  if (kStackOvfRows > 0 &&
      hipMalloc(reinterpret_cast<void**>(&c->stackOvf), (size_t)kStackOvfRows * c->stackOvfStride * sizeof(int)) != hipSuccess) {
    bdpt_destroy(c);
    return BDPT_E_NOMEM;
  }
  if (hipMalloc(reinterpret_cast<void**>(&c->rayCursor), 2 * sizeof(unsigned long long)) != hipSuccess ||
      hipMemset(c->rayCursor, 0, 2 * sizeof(unsigned long long)) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&c->adaptiveSum), 2 * sizeof(unsigned long long)) != hipSuccess ||
      hipMemset(c->adaptiveSum, 0, 2 * sizeof(unsigned long long)) != hipSuccess) {
    bdpt_destroy(c);
    return BDPT_E_NOMEM;
  }
  bvhPrewarmStaging(device_ordinal);  // (the pinned staging buffers bdpt_set_scene's uploads go through)
  *out_ctx = c;
  return BDPT_OK;
}

void bdpt_destroy(bdpt_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  if (c->stackOvf) (void)hipFree(c->stackOvf);
  if (c->rayCursor) (void)hipFree(c->rayCursor);
  if (c->adaptiveSum) (void)hipFree(c->adaptiveSum);
  freeLightGroups(c);
  freeBmfrHistory(c->bmfr);
  freeBmfrHistory(c->bmfrPlanes);
  freePool(c->sceneAllocs);
  freePool(c->skinAllocs);
  freePool(c->morphAllocs);
  freePool(c->frameAllocs);
  if (c->evCreated)
    for (int i = 0; i <= kMaxStages; i++) (void)hipEventDestroy(c->ev[i]);
  if (c->evCreated)
    for (hipEvent_t e : c->sideEv) (void)hipEventDestroy(e);
  if (c->evFork) (void)hipEventDestroy(c->evFork);
  if (c->evJoin) (void)hipEventDestroy(c->evJoin);
  if (c->evSplat) (void)hipEventDestroy(c->evSplat);
  if (c->evStage) (void)hipEventDestroy(c->evStage);
  if (c->evOrder) (void)hipEventDestroy(c->evOrder);
  if (c->pinned) (void)hipHostFree(c->pinned);
  if (c->walkStream) (void)hipStreamDestroy(c->walkStream);
  delete c;
}

const char* bdpt_last_error(const bdpt_ctx* c) { return c ? c->err.c_str() : "null context"; }

// The scene's acceleration structure built on `device` (bvh_device.hip: references, binary tree, collapse and packed
// records — the records the host code produces, bit for bit).  The one place that reads the build's measurement knobs,
// at every call: BDPT_HOST_PRIORITIES (the host decides what the clipper leaves, priorities and split counts),
// BDPT_UPLOAD_TRI_RECS (the host's triangle records and boxes are uploaded).
static void buildSceneBvhOnDevice(const bdpt_scene_desc* d, int device, bool classify, SceneBvh& sb, std::string& error) {
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

static int setSceneImpl(bdpt_ctx* c, const bdpt_scene_desc* d) {
  if (!c || !d) return BDPT_E_INVALID;
  if (!d->positions || !d->normals || !d->indices || !d->triMaterial || !d->materials || !d->numMaterials) {
    fail(c, "scene: positions, normals, indices, triMaterial and materials are required");
    return BDPT_E_INVALID;
  }
  if (d->numLights == 0 || !d->lights) {
    fail(c, "scene: at least one light is required (SceneLoaderWrapper adds a directional light when a file has none)");
    return BDPT_E_INVALID;
  }
  if (d->numLights > BDPT_MAX_LIGHTS) {
    fail(c, "scene: more than BDPT_MAX_LIGHTS lights");
    return BDPT_E_LIMIT;
  }
  if (d->numTriangles >= (1u << 28)) {
    fail(c, "scene: triangle count exceeds the 2^28 leaf-reference limit");
    return BDPT_E_LIMIT;
  }
  {
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
    if (bad.load() == 3) {
      fail(c, "scene: a triangle has a vertex position that is not finite or lies beyond 2^60");
      return BDPT_E_INVALID;
    }
    if (bad.load() == 1) {
      fail(c, "scene: triMaterial out of range");
      return BDPT_E_INVALID;
    }
    if (bad.load() == 2) {
      fail(c, "scene: vertex index out of range");
      return BDPT_E_INVALID;
    }
  }
  for (uint32_t m = 0; m < d->numMaterials; m++) {
    const bdpt_material& mm = d->materials[m];
    const int ids[4] = {mm.texBaseColor, mm.texSpecular, mm.texEmissive, mm.texNormal};
    for (int id : ids)
      if (id < -1 || id >= (int)d->numTextures) {
        fail(c, "scene: material texture index out of range");
        return BDPT_E_INVALID;
      }
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  freePool(c->sceneAllocs);
  freePool(c->skinAllocs);
  c->haveSkin = false;
  c->skin = SkinDev{};
  c->skinPalette[0] = c->skinPalette[1] = nullptr;
  dropMorph(c);
  freeLightGroups(c);
  c->haveScene = false;
  c->S = SceneDev{};
  c->refitReady = false;
  c->refitPlan = BvhRefitPlan{};
  c->refit = RefitDev{};
  c->numUpdates = 0;
  c->lightMaps = nullptr;
  c->alphaTris = nullptr;
  c->numAlphaTris = 0;
  c->areaReady = false;
  c->area = AreaDev{};
  c->areaTextured = 0;
  c->areaBlockSum = nullptr;
  c->areaBlockLast = nullptr;
  c->prevPose = nullptr;
  for (float*& p : c->stage) p = nullptr;
  c->stageInFlight = false;
  c->S.stackOvf = c->stackOvf;
  c->S.stackOvfStride = c->stackOvfStride;

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
  // Beside the build, on a thread of its own: the per-primitive shading records (3 x (position, normal, uv) + material id,
  // 112 B in a 128-byte slot) and the uploads that depend on nothing the build produces — while the build's device stages run the host is
  // idle, and while its host stages run the copy engine is.
  struct SideUploads {
    std::vector<void*> pool;
    const float* shade = nullptr;
    const uint32_t* indices = nullptr;
    const float* bitangents = nullptr;
    hipError_t err = hipSuccess;
    std::string what;  // the staged upload's own message, when that is what failed
  };
  // (BDPT_SET_SCENE_SERIAL: measurement knob — the same work at the point where its results are needed, on this thread)
  std::future<SideUploads> side = std::async(std::getenv("BDPT_SET_SCENE_SERIAL") ? std::launch::deferred : std::launch::async, [c, d]() {
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
      u.pool.push_back(q);
      if (count) {
        std::string e;
        if (!bvhUploadStaged(q, host, count * sizeof(**dst), e)) {
          u.err = hipErrorUnknown;
          u.what = e;
        }
      }
      *dst = static_cast<std::remove_reference_t<decltype(*dst)>>(q);
    };
    u.err = hipSetDevice(c->device);
    up(&u.shade, shade.data(), shade.size());
    up(&u.indices, d->indices, (size_t)d->numTriangles * 3);
    if (d->bitangents) up(&u.bitangents, d->bitangents, (size_t)d->numVertices * 3);
    return u;
  });
  struct SideJoin {  // whatever way this function is left, the thread is joined and what it allocated has an owner
    std::future<SideUploads>& f;
    ~SideJoin() {
      if (!f.valid()) return;
      try {
        SideUploads u = f.get();
        for (void* q : u.pool) (void)hipFree(q);
      } catch (...) {
      }
    }
  } sideJoin{side};
  // traversal flags, alpha classification, spatial pre-splitting and the tree itself: scene_bvh.cpp
  SceneBvh sb;
  try {
    std::string treeError;
    buildSceneBvhOnDevice(d, c->device, std::getenv("BDPT_NO_ALPHA_CLASSIFY") == nullptr, sb, treeError);
    if (sb.bvh.deviceRecs) c->sceneAllocs.push_back(sb.bvh.deviceRecs);  // (the context's from here on)
    if (!treeError.empty()) {
      fail(c, "scene: " + treeError);
      return treeError.find("2^31") != std::string::npos ? BDPT_E_LIMIT : (treeError.find("out of device memory") != std::string::npos ? BDPT_E_NOMEM : BDPT_E_HIP);
    }
  } catch (const std::bad_alloc&) {
    fail(c, "scene: out of host memory while building the acceleration structure");
    return BDPT_E_NOMEM;
  }
  lap("buildSceneBvh");
  Bvh& bvh = sb.bvh;
  const std::vector<uint32_t>& alphaTris = sb.alphaTris;
  if (bvh.maxStack > (uint32_t)kBvhMaxStack) {
    fail(c, "bvh needs a deeper traversal stack than the device provides");
    return BDPT_E_LIMIT;
  }
  if (!bvh.deviceRecs && !bvh.recs.empty()) {  // nothing to build a tree over (no triangle can be hit): the host's one empty node
    const BvhRec* dRecs = nullptr;
    if (int rc0 = devUpload(c, c->sceneAllocs, &dRecs, bvh.recs.data(), bvh.recs.size())) return rc0;
    bvh.deviceRecs = const_cast<BvhRec*>(dRecs);
    bvh.deviceNumRecs = bvh.recs.size();
  }
  if (!bvh.deviceRecs) {
    fail(c, "scene: the acceleration structure has no records");
    return BDPT_E_HIP;
  }
  c->bvhInfo.numNodes = bvh.numNodes;
  c->bvhInfo.numTriangles = d->numTriangles;
  c->bvhInfo.maxDepth = bvh.maxDepth;
  c->bvhInfo.nodeBytes = sizeof(BvhRec);
  c->bvhInfo.triBytes = sizeof(BvhTri);
  c->bvhInfo.sahCost = bvh.sahCost;
  c->bvhInfo.maxStack = bvh.maxStack;
  c->bvhInfo.numReferences = bvh.numRefs;
  c->bvhInfo.numDropped = bvh.numDropped;
  c->bvhInfo.numAlphaMode = sb.numAlphaMode;
  c->bvhInfo.numAlwaysPass = sb.numAlwaysPass;

  int rc;
  {
    SideUploads u = side.get();  // (a std::bad_alloc of that thread is rethrown here: bdpt_set_scene's catch)
    c->sceneAllocs.insert(c->sceneAllocs.end(), u.pool.begin(), u.pool.end());
    if (u.err != hipSuccess) {
      fail(c, std::string("scene upload: ") + (u.what.empty() ? std::string(hipGetErrorString(u.err)) : u.what));
      return u.err == hipErrorOutOfMemory ? BDPT_E_NOMEM : BDPT_E_HIP;
    }
    c->S.shade = reinterpret_cast<const float4*>(u.shade);
    c->S.indices = u.indices;
    if (d->bitangents) {
      c->S.bitangents = u.bitangents;
      c->S.hasBitangents = 1;
    }
  }
  lap("shading records + uploads (joined)");
  c->S.recs = reinterpret_cast<const uint4*>(bvh.deviceRecs);
  c->S.numRecs = (uint32_t)bvh.deviceNumRecs;
  if ((rc = devUpload(c, c->sceneAllocs, &c->S.materials, d->materials, d->numMaterials))) return rc;
  std::vector<TexDev> texs(d->numTextures);
  for (uint32_t i = 0; i < d->numTextures; i++) {
    const bdpt_texture& t = d->textures[i];
    if (!t.rgba8 || !t.width || !t.height) {
      fail(c, "scene: empty texture");
      return BDPT_E_INVALID;
    }
    // one spare texel after the last: the row-pair load of the last texel (device_scene.hpp texelRow) stays inside
    const size_t bytes = (size_t)t.width * t.height * 4;
    uint8_t* px = nullptr;
    if ((rc = devAlloc(c, c->sceneAllocs, &px, bytes + 4))) return rc;
    HIPCHK(c, hipMemset(px + bytes, 0, 4));
    {
      std::string e;
      if (!bvhUploadStaged(px, t.rgba8, bytes, e)) {
        fail(c, e);
        return BDPT_E_HIP;
      }
    }
    texs[i] = TexDev{px, t.width, t.height, t.srgb, texPow2Flags(t.width, t.height)};
  }
  if ((rc = devUpload(c, c->sceneAllocs, &c->S.textures, texs.data(), texs.size()))) return rc;
  {
    std::vector<TexDev> matTex((size_t)d->numMaterials * 4, TexDev{nullptr, 0, 0, 0, 0});
    for (uint32_t mi = 0; mi < d->numMaterials; mi++) {
      const bdpt_material& mm = d->materials[mi];
      const int ids[4] = {mm.texBaseColor, mm.texSpecular, mm.texEmissive, mm.texNormal};
      for (int k = 0; k < 4; k++)
        if (ids[k] >= 0) matTex[(size_t)mi * 4 + k] = texs[(size_t)ids[k]];
    }
    if ((rc = devUpload(c, c->sceneAllocs, &c->S.matTex, matTex.data(), matTex.size()))) return rc;
  }
  {
    // the alpha-test records of the non-opaque triangles, made on the device from the shading records and the material
    // tables already there (kernels.hip alpha_recs_kernel): only the list of those triangles crosses the bus
    float4* dAlpha = nullptr;
    if ((rc = devAlloc(c, c->sceneAllocs, &dAlpha, std::max<size_t>(alphaTris.size(), 1) * 4))) return rc;
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
        if ((rc = devUpload(c, c->sceneAllocs, &dPlane, plane.data(), plane.size()))) return rc;
        quadByTex[(size_t)mm.texBaseColor] = (unsigned long long)reinterpret_cast<uintptr_t>(dPlane);
      }
      const uint32_t* dList = nullptr;
      const unsigned long long* dQuad = nullptr;
      std::vector<void*> scratch;
      // (the list stays: the emitter table of area lights finds a triangle's alpha-test record in it)
      if ((rc = devUpload(c, c->sceneAllocs, &dList, alphaTris.data(), alphaTris.size())) ||
          (rc = devUpload(c, scratch, &dQuad, quadByTex.data(), quadByTex.size()))) {
        freePool(scratch);
        return rc;
      }
      c->alphaTris = dList;
      c->numAlphaTris = (uint32_t)alphaTris.size();
      launchAlphaRecs(c->S, dList, (uint32_t)alphaTris.size(), dQuad, dAlpha, nullptr);
      const hipError_t e = hipDeviceSynchronize();
      freePool(scratch);
      HIPCHK(c, e);
    }
    c->S.alphaRecs = dAlpha;
  }
  lap("indices, textures, alpha");
  SceneConst sc;
  std::memset(&sc, 0, sizeof(sc));
  std::memcpy(sc.lights, d->lights, sizeof(bdpt_light) * d->numLights);
  for (int i = 0; i < 256; i++) {
    double cc = (double)i / 255.0;
    double l = (cc <= 0.04045) ? cc / 12.92 : std::pow((cc + 0.055) / 1.055, 2.4);
    sc.srgbLut[i] = (float)l;
  }
  if ((rc = devUpload(c, c->sceneAllocs, &c->S.sc, &sc, 1))) return rc;
  c->S.numLights = d->numLights;
  // Occluder hints of next-event rays: one cube map of nearest triangles per light (directional lights: empty), traced
  // here once; the primary-visibility hints of an earlier scene index records that are gone.
  c->hints = std::getenv("BDPT_NO_HINTS") == nullptr;
  if (c->hints) {
    uint32_t res = 512;
    if (const char* e = std::getenv("BDPT_LIGHT_MAP_RES")) res = (uint32_t)std::max(0, std::min(2048, std::atoi(e)));
    if (res) {
      uint32_t* maps = nullptr;
      if ((rc = devAlloc(c, c->sceneAllocs, &maps, (size_t)6 * res * res * d->numLights))) return rc;
      launchLightMaps(c->S, maps, res, nullptr);
      HIPCHK(c, hipDeviceSynchronize());
      c->S.lightMap = maps;
      c->S.lightMapRes = res;
      c->lightMaps = maps;
    }
  }
  if (c->hintPix) HIPCHK(c, hipMemset(c->hintPix, 0xFF, (size_t)c->W * c->H * sizeof(uint32_t)));
  c->hintCamValid = false;
  lap("light maps");
  c->numVertices = d->numVertices;
  c->numTriangles = d->numTriangles;
  c->haveScene = true;
  return BDPT_OK;
}
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
  if (!c->haveScene) return BDPT_E_STATE;
  *out = c->bvhInfo;
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
  if (env && env->envMap && (!env->width || !env->height)) {
    fail(c, "environment: a map needs a width and a height");
    return BDPT_E_INVALID;
  }
  c->env = env ? *env : bdpt_environment{};
  if (!c->env.envMap) c->env.width = c->env.height = 0;
  return BDPT_OK;
}

// ---- animated scenes: refit in place (refit.hip, bvh.h "refit") ----
namespace {
// host arrays -> pinned memory (now) -> device copies (on st); arrays[k] may be null
int stageHostArrays(bdpt_ctx* c, const void* const* arrays, const size_t* bytes, int n, float** dst, hipStream_t st) {
  size_t total = 0;
  for (int k = 0; k < n; k++) total += arrays[k] ? (bytes[k] + 255) / 256 * 256 : 0;
  if (c->stageInFlight) HIPCHK(c, hipEventSynchronize(c->evStage));  // the copies of the last update have read the buffer
  c->stageInFlight = false;
  if (total > c->pinnedBytes) {
    if (c->pinned) HIPCHK(c, hipHostFree(c->pinned));
    c->pinned = nullptr;
    c->pinnedBytes = 0;
    if (hipHostMalloc(&c->pinned, total, hipHostMallocDefault) != hipSuccess) {
      fail(c, "update: pinned staging memory");
      return BDPT_E_NOMEM;
    }
    c->pinnedBytes = total;
  }
  size_t off = 0;
  for (int k = 0; k < n; k++) {
    if (!arrays[k]) continue;
    std::memcpy(static_cast<char*>(c->pinned) + off, arrays[k], bytes[k]);
    HIPCHK(c, hipMemcpyAsync(dst[k], static_cast<char*>(c->pinned) + off, bytes[k], hipMemcpyHostToDevice, st));
    off += (bytes[k] + 255) / 256 * 256;
  }
  HIPCHK(c, hipEventRecord(c->evStage, st));
  c->stageInFlight = true;
  return BDPT_OK;
}
// the light cube maps of the occluder hints, re-traced on st
void retraceLightMaps(bdpt_ctx* c, hipStream_t st) {
  if (c->hints && c->lightMaps) launchLightMaps(c->S, c->lightMaps, c->S.lightMapRes, st);
}

// What every update ends with, on st: the refit to the device arrays `pos` (and `nrm`), the emitter table's refresh, the
// bitangent copy, the light maps' re-trace unless kept.
int updateTail(bdpt_ctx* c, const float* pos, const float* nrm, const float* bit, uint32_t flags, hipStream_t st) {
  const size_t nv3 = (size_t)c->numVertices * 3;
  launchRefit(c->refit, reinterpret_cast<BvhRec*>(const_cast<uint4*>(c->S.recs)), const_cast<float4*>(c->S.shade), c->S.indices, c->numTriangles, pos, nrm, st);
  if (c->areaReady) launchAreaRefresh(c->S, c->area, c->areaBlockSum, c->areaBlockLast, st);  // weights and CDF of the new areas
  if (bit) HIPCHK(c, hipMemcpyAsync(const_cast<float*>(c->S.bitangents), bit, nv3 * 4, hipMemcpyDeviceToDevice, st));
  if (!(flags & BDPT_UPDATE_KEEP_LIGHT_MAPS)) retraceLightMaps(c, st);
  HIPCHK(c, hipGetLastError());
  c->hintCamValid = false;
  c->numUpdates++;
  c->lastStream = st;
  return BDPT_OK;
}
}  // namespace

int bdpt_update_geometry(bdpt_ctx* c, const bdpt_geometry_update* u, void* stream) {
  if (!c || !u) return BDPT_E_INVALID;
  if (!c->haveScene) {
    fail(c, "update: no scene (bdpt_set_scene first)");
    return BDPT_E_STATE;
  }
  if (!u->positions || u->numVertices != c->numVertices || u->memory > BDPT_MEMORY_DEVICE || (u->flags & ~BDPT_UPDATE_KEEP_LIGHT_MAPS)) {
    fail(c, u->numVertices != c->numVertices ? "update: numVertices differs from the scene's" : "update: positions missing or bad memory / flags");
    return BDPT_E_INVALID;
  }
  if (u->bitangents && !c->S.hasBitangents) {
    fail(c, "update: bitangents given for a scene that has none");
    return BDPT_E_INVALID;
  }
  const size_t nv3 = (size_t)c->numVertices * 3;
  if (u->memory == BDPT_MEMORY_HOST) {
    std::atomic<int> bad{0};
    hostParallelFor(nv3, [&](size_t i0, size_t i1) {
      for (size_t i = i0; i < i1; i++)
        if (!bvhCoordInRange(u->positions[i])) {  // (bvh.h kBvhMaxCoord; false for a NaN)
          bad.store(1);
          return;
        }
    });
    if (bad.load()) {
      fail(c, "update: a vertex position is not finite or lies beyond 2^60");
      return BDPT_E_INVALID;
    }
  }
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = ensureRefit(c, st)) return rc;
  const float* pos = u->positions;
  const float* nrm = u->normals;
  const float* bit = u->bitangents;
  if (u->memory == BDPT_MEMORY_HOST) {
    const float* in[3] = {u->positions, u->normals, u->bitangents};
    for (int k = 0; k < 3; k++)
      if (in[k] && !c->stage[k]) {
        if (streamIsCapturing(st)) {
          fail(c, "update: host-pointer inputs allocate their device copies on first use: not while capturing");
          return BDPT_E_STATE;
        }
        if (int rc = devAlloc(c, c->sceneAllocs, &c->stage[k], nv3)) return rc;
      }
    if (int rc = orderAfterLast(c, st)) return rc;
    const void* arrays[3] = {in[0], in[1], in[2]};
    const size_t bytes[3] = {nv3 * 4, nv3 * 4, nv3 * 4};
    if (int rc = stageHostArrays(c, arrays, bytes, 3, c->stage, st)) return rc;
    pos = c->stage[0];
    nrm = in[1] ? c->stage[1] : nullptr;
    bit = in[2] ? c->stage[2] : nullptr;
  } else {
    if (int rc = orderAfterLast(c, st)) return rc;
  }
  return updateTail(c, pos, nrm, bit, u->flags, st);
}

// ---- skinning and morph targets: bdpt_set_skin / bdpt_set_morph, one deformation pass behind bdpt_update_skinned and
// bdpt_update_morphed (deform.hip), and the same arithmetic on the host ----
namespace {
// the checks of a bdpt_skin_desc that need no context; `what` prefixes the message
int checkSkinDesc(bdpt_ctx* c, const bdpt_skin_desc* d, const char* what) {
  const std::string w(what);
  if (!d->positions || !d->boneWeights || !d->boneIds || d->reserved[0] || d->reserved[1] || d->numBones == 0) {
    fail(c, w + ": positions, boneWeights and boneIds are required, numBones >= 1 and reserved 0");
    return BDPT_E_INVALID;
  }
  if (d->numBones > BDPT_MAX_BONES) {
    fail(c, w + ": more than BDPT_MAX_BONES bones");
    return BDPT_E_LIMIT;
  }
  std::atomic<int> bad{0};  // 1 = position, 2 = weight, 3 = id
  hostParallelFor(d->numVertices, [&](size_t v0, size_t v1) {
    for (size_t v = v0; v < v1; v++) {
      const float* p = d->positions + v * 3;
      const float* wt = d->boneWeights + v * 4;
      if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) bad.store(1);
      if (!(std::isfinite(wt[0]) && std::isfinite(wt[1]) && std::isfinite(wt[2]) && std::isfinite(wt[3]))) {
        bad.store(2);
        continue;
      }
      if (skinIsStatic(wt)) continue;  // (its ids are neither checked nor read)
      for (int k = 0; k < 4; k++)
        if (d->boneIds[v * 4 + (size_t)k] >= d->numBones) bad.store(3);
    }
  });
  if (bad.load()) {
    fail(c, w + (bad.load() == 1 ? ": a rest position is not finite" : bad.load() == 2 ? ": a bone weight is not finite" : ": a bone id >= numBones on a vertex with a weight"));
    return BDPT_E_INVALID;
  }
  return BDPT_OK;
}

// The vertex loop of bdpt_host_skin and bdpt_host_morph: the base (with a skin, its rest pose), morphed if `m`, then
// skinned, or copied for a static vertex and without a skin.
void hostDeform(size_t numVertices, const float* baseP, const float* baseN, const float* baseB, const MorphCsr* m, const float* weights,
                const bdpt_skin_desc* skin, const float* bones, const float* normalBones, float* outP, float* outN, float* outB) {
  const float* dN = m && !m->dNrm.empty() ? m->dNrm.data() : nullptr;
  const float* dB = m && !m->dBit.empty() ? m->dBit.data() : nullptr;
  withFlag(baseN != nullptr, [&](auto hasN) {
    withFlag(baseB != nullptr, [&](auto hasB) {
      constexpr bool N = decltype(hasN)::value, B = decltype(hasB)::value;
      hostParallelFor(numVertices, [&](size_t v0, size_t v1) {
        for (size_t v = v0; v < v1; v++) {
          const size_t o = v * 3;
          float p[3], n[3] = {0.0f, 0.0f, 0.0f}, b[3] = {0.0f, 0.0f, 0.0f};
          for (int k = 0; k < 3; k++) {
            p[k] = baseP[o + k];
            if (N) n[k] = baseN[o + k];
            if (B) b[k] = baseB[o + k];
          }
          if (m) morphVertex(m->target.data(), m->dPos.data(), dN, dB, weights, m->start[v], m->start[v + 1], p, n, b);
          const float* w = skin ? skin->boneWeights + v * 4 : nullptr;
          if (skin && !skinIsStatic(w)) {
            skinVertex<N, B>(bones, normalBones, skin->boneIds + v * 4, w, p, n, b, outP + o, N ? outN + o : nullptr, B ? outB + o : nullptr);
            continue;
          }
          for (int k = 0; k < 3; k++) {
            outP[o + k] = p[k];
            if (N) outN[o + k] = n[k];
            if (B) outB[o + k] = b[k];
          }
        }
      });
    });
  });
}

// the context's deformed streams: the skin's with a skin, the morph's without
struct DeformOut {
  float *pos, *nrm, *bit;
};
DeformOut deformOut(const bdpt_ctx* c) {
  return c->haveSkin ? DeformOut{c->skin.pos, c->skin.nrm, c->skin.bit} : DeformOut{c->morph.pos, c->morph.nrm, c->morph.bit};
}
int deformedBuffers(const bdpt_ctx* c, const float** positions, const float** normals, const float** bitangents) {
  const DeformOut o = deformOut(c);
  *positions = o.pos;
  *normals = o.nrm;
  *bitangents = o.bit;
  return BDPT_OK;
}

// What bdpt_update_skinned (weights null) and bdpt_update_morphed do with arguments that passed their checks: the
// finiteness scan of host inputs, their staging, the deformation pass and the refit.  `what` prefixes the messages.
int updateDeformed(bdpt_ctx* c, const char* what, const float* weights, const float* bones, const float* nbones, uint32_t memory, uint32_t flags,
                   void* stream) {
  const std::string w(what);
  const MorphDev* M = weights ? &c->morph : nullptr;
  const SkinDev* K = c->haveSkin ? &c->skin : nullptr;
  const size_t nw = M ? M->numTargets : 0, pal = K ? (size_t)K->numBones * 16 : 0;
  const bool host = memory == BDPT_MEMORY_HOST;
  if (host) {
    bool finite = true;
    for (size_t t = 0; t < nw; t++) finite = finite && std::isfinite(weights[t]);
    for (size_t i = 0; i < pal; i++) finite = finite && std::isfinite(bones[i]) && (!nbones || std::isfinite(nbones[i]));
    if (!finite) {
      fail(c, w + (M ? ": a weight or a bone matrix element is not finite" : ": a bone matrix element is not finite"));
      return BDPT_E_INVALID;
    }
  }
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = ensureRefit(c, st)) return rc;  // (bdpt_set_skin / bdpt_set_morph made the plan: nothing to do)
  if (host && streamIsCapturing(st)) {
    fail(c, w + ": host-pointer " + (M ? "weights and palettes" : "palettes") + " are staged through pinned memory: not while capturing");
    return BDPT_E_STATE;
  }
  if (int rc = orderAfterLast(c, st)) return rc;
  if (host) {
    const void* arrays[3] = {weights, bones, nbones};
    const size_t bytes[3] = {nw * 4, pal * 4, pal * 4};
    float* dst[3] = {c->morphWeights, c->skinPalette[0], c->skinPalette[1]};
    if (int rc = stageHostArrays(c, arrays, bytes, 3, dst, st)) return rc;
    if (weights) weights = dst[0];
    if (bones) bones = dst[1];
    if (nbones) nbones = dst[2];
  }
  launchDeform(M, weights, K, bones, nbones, kSkinPathAuto, st);
  const DeformOut o = deformOut(c);
  return updateTail(c, o.pos, o.nrm, o.bit, flags, st);
}

// bdpt_test_skin_kernel and bdpt_test_morph_kernel: the pass alone, with the palettes (and weights) of the last update
int testDeformKernel(bdpt_ctx* c, bool morph, uint32_t path, void* stream) {
  if (!c || path > (uint32_t)kSkinPathLds) return BDPT_E_INVALID;
  if (!c->haveScene || !(morph ? c->haveMorph : c->haveSkin)) {
    fail(c, morph ? "test_morph_kernel: no morph (bdpt_set_morph first)" : "test_skin_kernel: no skin (bdpt_set_skin first)");
    return BDPT_E_STATE;
  }
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = orderAfterLast(c, st)) return rc;
  // (skinPalette[k] is null where the context has no skin, or its skin no normals)
  launchDeform(morph ? &c->morph : nullptr, c->morphWeights, c->haveSkin ? &c->skin : nullptr, c->skinPalette[0], c->skinPalette[1], (int)path, st);
  HIPCHK(c, hipGetLastError());
  c->lastStream = st;
  return BDPT_OK;
}
}  // namespace

int bdpt_host_skin(const bdpt_skin_desc* d, const float* bones, const float* normalBones, float* outPositions, float* outNormals,
                   float* outBitangents) {
  if (!d || !bones || !outPositions) return BDPT_E_INVALID;
  if ((d->normals && (!normalBones || !outNormals)) || (d->bitangents && !outBitangents)) return BDPT_E_INVALID;
  if (int rc = checkSkinDesc(nullptr, d, "host_skin")) return rc;
  hostDeform(d->numVertices, d->positions, d->normals, d->bitangents, nullptr, nullptr, d, bones, normalBones, outPositions, outNormals, outBitangents);
  return BDPT_OK;
}

int bdpt_set_skin(bdpt_ctx* c, const bdpt_skin_desc* d) {
  if (!c) return BDPT_E_INVALID;
  if (!c->haveScene) {
    fail(c, "set_skin: no scene (bdpt_set_scene first)");
    return BDPT_E_STATE;
  }
  if (d) {
    if (d->numVertices != c->numVertices) {
      fail(c, "set_skin: numVertices differs from the scene's");
      return BDPT_E_INVALID;
    }
    if (d->bitangents && !c->S.hasBitangents) {
      fail(c, "set_skin: bitangents given for a scene that has none");
      return BDPT_E_INVALID;
    }
    if (int rc = checkSkinDesc(c, d, "set_skin")) return rc;
  }
  ENTER(c);
  if (streamIsCapturing(c->lastStream)) {
    fail(c, "set_skin: not inside a stream capture (it allocates and synchronises)");
    return BDPT_E_STATE;
  }
  if (d)
    if (int rc = ensureRefit(c, c->lastStream)) return rc;  // (before the old skin goes: a failure leaves it in place)
  HIPCHK(c, hipDeviceSynchronize());
  std::vector<void*> pool;
  SkinDev K{};
  float* palette[2] = {nullptr, nullptr};
  if (d) {
    const size_t nv = d->numVertices, nv3 = nv * 3, pal = (size_t)d->numBones * 16;
    int rc;
    if ((rc = devUpload(c, pool, &K.restPos, d->positions, nv3)) || (d->normals && (rc = devUpload(c, pool, &K.restNrm, d->normals, nv3))) ||
        (d->bitangents && (rc = devUpload(c, pool, &K.restBit, d->bitangents, nv3))) || (rc = devUpload(c, pool, &K.weights, d->boneWeights, nv * 4)) ||
        (rc = devUpload(c, pool, &K.ids, d->boneIds, nv * 4)) || (rc = devAlloc(c, pool, &K.pos, nv3)) ||
        (d->normals && (rc = devAlloc(c, pool, &K.nrm, nv3))) || (d->bitangents && (rc = devAlloc(c, pool, &K.bit, nv3))) ||
        (rc = devAlloc(c, pool, &palette[0], pal)) || (d->normals && (rc = devAlloc(c, pool, &palette[1], pal)))) {
      freePool(pool);
      return rc;
    }
    // until the first update the skinned streams hold the rest pose, the palettes zeros
    hipError_t e = hipMemcpy(K.pos, K.restPos, nv3 * 4, hipMemcpyDeviceToDevice);
    if (e == hipSuccess && K.nrm) e = hipMemcpy(K.nrm, K.restNrm, nv3 * 4, hipMemcpyDeviceToDevice);
    if (e == hipSuccess && K.bit) e = hipMemcpy(K.bit, K.restBit, nv3 * 4, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipMemset(palette[0], 0, pal * 4);
    if (e == hipSuccess && palette[1]) e = hipMemset(palette[1], 0, pal * 4);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
      freePool(pool);
      fail(c, std::string("set_skin: ") + hipGetErrorString(e));
      return BDPT_E_HIP;
    }
    K.numVertices = d->numVertices;
    K.numBones = d->numBones;
  }
  dropMorph(c);  // (its base and its outputs were this skin's, or it had none: scene, skin, morph is the order)
  freePool(c->skinAllocs);
  c->skinAllocs = std::move(pool);
  c->skin = K;
  c->skinPalette[0] = palette[0];
  c->skinPalette[1] = palette[1];
  c->haveSkin = d != nullptr;
  return BDPT_OK;
}

int bdpt_update_skinned(bdpt_ctx* c, const bdpt_skin_update* u, void* stream) {
  if (!c || !u) return BDPT_E_INVALID;
  if (!c->haveScene || !c->haveSkin) {
    fail(c, c->haveScene ? "update_skinned: no skin (bdpt_set_skin first)" : "update_skinned: no scene (bdpt_set_scene first)");
    return BDPT_E_STATE;
  }
  const SkinDev& K = c->skin;
  if (!u->bones || (K.nrm && !u->normalBones) || u->numBones != K.numBones || u->memory > BDPT_MEMORY_DEVICE ||
      (u->flags & ~BDPT_UPDATE_KEEP_LIGHT_MAPS) || u->reserved) {
    fail(c, u->numBones != K.numBones ? "update_skinned: numBones differs from the skin's"
                                      : "update_skinned: bones (or normalBones, for a skin with normals) missing, or bad memory / flags / reserved");
    return BDPT_E_INVALID;
  }
  return updateDeformed(c, "update_skinned", nullptr, u->bones, K.nrm ? u->normalBones : nullptr, u->memory, u->flags, stream);
}

int bdpt_skinned_buffers(bdpt_ctx* c, const float** positions, const float** normals, const float** bitangents) {
  if (!c || !positions || !normals || !bitangents) return BDPT_E_INVALID;
  if (!c->haveScene || !c->haveSkin) {
    fail(c, "skinned_buffers: no skin (bdpt_set_skin first)");
    return BDPT_E_STATE;
  }
  return deformedBuffers(c, positions, normals, bitangents);
}

int bdpt_test_skin_kernel(bdpt_ctx* c, uint32_t path, void* stream) { return testDeformKernel(c, false, path, stream); }
int bdpt_test_morph_kernel(bdpt_ctx* c, uint32_t path, void* stream) { return testDeformKernel(c, true, path, stream); }

namespace {
// The checks of a bdpt_morph_desc.  haveSkin: the base is a skin's rest pose, which has normals / bitangents where
// skinN / skinB; `what` prefixes the message.
int checkMorphDesc(bdpt_ctx* c, const bdpt_morph_desc* d, bool haveSkin, bool skinN, bool skinB, const char* what) {
  const std::string w(what);
  if (!d->targetStart || !d->vertex || !d->dPositions || d->reserved[0] || d->reserved[1] || d->numTargets == 0) {
    fail(c, w + ": targetStart, vertex and dPositions are required, numTargets >= 1 and reserved 0");
    return BDPT_E_INVALID;
  }
  if (d->numTargets > BDPT_MAX_MORPH_TARGETS) {
    fail(c, w + ": more than BDPT_MAX_MORPH_TARGETS targets");
    return BDPT_E_LIMIT;
  }
  if (haveSkin) {
    if (d->positions || d->normals || d->bitangents) {
      fail(c, w + ": the base is the skin's rest pose: positions, normals and bitangents must be NULL");
      return BDPT_E_INVALID;
    }
  } else if (!d->positions) {
    fail(c, w + ": positions (the base pose) are required without a skin");
    return BDPT_E_INVALID;
  }
  if ((d->dNormals && !(haveSkin ? skinN : d->normals != nullptr)) || (d->dBitangents && !(haveSkin ? skinB : d->bitangents != nullptr))) {
    fail(c, w + ": deltas for a stream the base lacks");
    return BDPT_E_INVALID;
  }
  if (d->targetStart[0] != 0) {
    fail(c, w + ": targetStart[0] is not 0");
    return BDPT_E_INVALID;
  }
  for (uint32_t t = 0; t < d->numTargets; t++)
    if (d->targetStart[t + 1] < d->targetStart[t]) {
      fail(c, w + ": targetStart decreases");
      return BDPT_E_INVALID;
    }
  const size_t ne = d->targetStart[d->numTargets];
  if (ne >= ((size_t)1 << 31)) {
    fail(c, w + ": 2^31 entries or more");
    return BDPT_E_LIMIT;
  }
  for (uint32_t t = 0; t < d->numTargets; t++)
    for (size_t e = d->targetStart[t]; e < d->targetStart[t + 1]; e++)
      if (d->vertex[e] >= d->numVertices || (e > d->targetStart[t] && d->vertex[e] <= d->vertex[e - 1])) {
        fail(c, w + ": a vertex id >= numVertices, or ids not strictly ascending within a target");
        return BDPT_E_INVALID;
      }
  std::atomic<int> bad{0};
  const float* deltas[3] = {d->dPositions, d->dNormals, d->dBitangents};
  const float* base[3] = {d->positions, d->normals, d->bitangents};
  for (int k = 0; k < 3; k++) {
    if (deltas[k])
      hostParallelFor(ne * 3, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++)
          if (!std::isfinite(deltas[k][i])) bad.store(1);
      });
    if (base[k])
      hostParallelFor((size_t)d->numVertices * 3, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++)
          if (!std::isfinite(base[k][i])) bad.store(2);
      });
  }
  if (bad.load()) {
    fail(c, w + (bad.load() == 1 ? ": a delta is not finite" : ": a base value is not finite"));
    return BDPT_E_INVALID;
  }
  return BDPT_OK;
}
}  // namespace

int bdpt_host_morph(const bdpt_morph_desc* d, const bdpt_skin_desc* skin, const float* weights, const float* bones, const float* normalBones,
                    float* outPositions, float* outNormals, float* outBitangents) {
  if (!d || !weights || !outPositions) return BDPT_E_INVALID;
  if (skin) {
    if (skin->numVertices != d->numVertices || !bones || (skin->normals && !normalBones)) return BDPT_E_INVALID;
    if (int rc = checkSkinDesc(nullptr, skin, "host_morph")) return rc;
  } else if (bones || normalBones) {
    return BDPT_E_INVALID;
  }
  if (int rc = checkMorphDesc(nullptr, d, skin != nullptr, skin && skin->normals, skin && skin->bitangents, "host_morph")) return rc;
  const float* baseP = skin ? skin->positions : d->positions;
  const float* baseN = skin ? skin->normals : d->normals;
  const float* baseB = skin ? skin->bitangents : d->bitangents;
  if ((baseN && !outNormals) || (baseB && !outBitangents)) return BDPT_E_INVALID;
  for (uint32_t t = 0; t < d->numTargets; t++)
    if (!std::isfinite(weights[t])) return BDPT_E_INVALID;
  const MorphCsr m = morphBuildCsr(d->numVertices, d->numTargets, d->targetStart, d->vertex, d->dPositions, d->dNormals, d->dBitangents);
  hostDeform(d->numVertices, baseP, baseN, baseB, &m, weights, skin, bones, normalBones, outPositions, outNormals, outBitangents);
  return BDPT_OK;
}

int bdpt_set_morph(bdpt_ctx* c, const bdpt_morph_desc* d) {
  if (!c) return BDPT_E_INVALID;
  if (!c->haveScene) {
    fail(c, "set_morph: no scene (bdpt_set_scene first)");
    return BDPT_E_STATE;
  }
  if (d) {
    if (d->numVertices != c->numVertices) {
      fail(c, "set_morph: numVertices differs from the scene's");
      return BDPT_E_INVALID;
    }
    if ((d->bitangents || d->dBitangents) && !c->S.hasBitangents) {
      fail(c, "set_morph: bitangents given for a scene that has none");
      return BDPT_E_INVALID;
    }
    if (int rc = checkMorphDesc(c, d, c->haveSkin, c->skin.nrm != nullptr, c->skin.bit != nullptr, "set_morph")) return rc;
  }
  ENTER(c);
  if (streamIsCapturing(c->lastStream)) {
    fail(c, "set_morph: not inside a stream capture (it allocates and synchronises)");
    return BDPT_E_STATE;
  }
  if (d)
    if (int rc = ensureRefit(c, c->lastStream)) return rc;  // (before the old morph goes: a failure leaves it in place)
  HIPCHK(c, hipDeviceSynchronize());
  std::vector<void*> pool;
  MorphDev M{};
  float* weights = nullptr;
  if (d) {
    const MorphCsr m = morphBuildCsr(d->numVertices, d->numTargets, d->targetStart, d->vertex, d->dPositions, d->dNormals, d->dBitangents);
    const size_t nv3 = (size_t)d->numVertices * 3;
    int rc;
    if ((rc = devUpload(c, pool, &M.start, m.start.data(), m.start.size())) || (rc = devUpload(c, pool, &M.target, m.target.data(), m.target.size())) ||
        (rc = devUpload(c, pool, &M.dPos, m.dPos.data(), m.dPos.size())) ||
        (d->dNormals && (rc = devUpload(c, pool, &M.dNrm, m.dNrm.data(), m.dNrm.size()))) ||
        (d->dBitangents && (rc = devUpload(c, pool, &M.dBit, m.dBit.data(), m.dBit.size()))) ||
        (rc = devUpload(c, pool, &M.active, m.active.data(), m.active.size())) || (rc = devAlloc(c, pool, &weights, d->numTargets)) ||
        (d->positions && ((rc = devUpload(c, pool, &M.basePos, d->positions, nv3)) || (rc = devAlloc(c, pool, &M.pos, nv3)))) ||
        (d->normals && ((rc = devUpload(c, pool, &M.baseNrm, d->normals, nv3)) || (rc = devAlloc(c, pool, &M.nrm, nv3)))) ||
        (d->bitangents && ((rc = devUpload(c, pool, &M.baseBit, d->bitangents, nv3)) || (rc = devAlloc(c, pool, &M.bit, nv3))))) {
      freePool(pool);
      return rc;
    }
    // until the first update the morphed streams hold the base, the weights zeros
    hipError_t e = hipMemset(weights, 0, (size_t)d->numTargets * 4);
    if (e == hipSuccess && M.pos) e = hipMemcpy(M.pos, M.basePos, nv3 * 4, hipMemcpyDeviceToDevice);
    if (e == hipSuccess && M.nrm) e = hipMemcpy(M.nrm, M.baseNrm, nv3 * 4, hipMemcpyDeviceToDevice);
    if (e == hipSuccess && M.bit) e = hipMemcpy(M.bit, M.baseBit, nv3 * 4, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
      freePool(pool);
      fail(c, std::string("set_morph: ") + hipGetErrorString(e));
      return BDPT_E_HIP;
    }
    M.numVertices = d->numVertices;
    M.numTargets = d->numTargets;
    M.numActive = (uint32_t)m.active.size();
  }
  dropMorph(c);
  c->morphAllocs = std::move(pool);
  c->morph = M;
  c->morphWeights = weights;
  c->haveMorph = d != nullptr;
  return BDPT_OK;
}

int bdpt_update_morphed(bdpt_ctx* c, const bdpt_morph_update* u, void* stream) {
  if (!c || !u) return BDPT_E_INVALID;
  if (!c->haveScene || !c->haveMorph) {
    fail(c, c->haveScene ? "update_morphed: no morph (bdpt_set_morph first)" : "update_morphed: no scene (bdpt_set_scene first)");
    return BDPT_E_STATE;
  }
  const MorphDev& M = c->morph;
  const SkinDev* K = c->haveSkin ? &c->skin : nullptr;
  const bool needN = K && K->nrm;
  if (!u->weights || u->numTargets != M.numTargets || u->numBones != (K ? K->numBones : 0u) || (u->bones != nullptr) != (K != nullptr) ||
      (u->normalBones != nullptr) != needN || u->memory > BDPT_MEMORY_DEVICE || (u->flags & ~BDPT_UPDATE_KEEP_LIGHT_MAPS) || u->reserved[0] ||
      u->reserved[1]) {
    fail(c, u->numTargets != M.numTargets ? "update_morphed: numTargets differs from the morph's"
            : u->numBones != (K ? K->numBones : 0u)
                ? "update_morphed: numBones differs from the skin's (0 without a skin)"
                : "update_morphed: weights missing, palettes missing with a skin or given without one, or bad memory / flags / reserved");
    return BDPT_E_INVALID;
  }
  return updateDeformed(c, "update_morphed", u->weights, u->bones, u->normalBones, u->memory, u->flags, stream);
}

int bdpt_morphed_buffers(bdpt_ctx* c, const float** positions, const float** normals, const float** bitangents) {
  if (!c || !positions || !normals || !bitangents) return BDPT_E_INVALID;
  if (!c->haveScene || !c->haveMorph) {
    fail(c, "morphed_buffers: no morph (bdpt_set_morph first)");
    return BDPT_E_STATE;
  }
  return deformedBuffers(c, positions, normals, bitangents);
}

int bdpt_set_lights(bdpt_ctx* c, const bdpt_light* lights, uint32_t numLights, void* stream) {
  if (!c || !lights) return BDPT_E_INVALID;
  if (!c->haveScene) {
    fail(c, "set_lights: no scene (bdpt_set_scene first)");
    return BDPT_E_STATE;
  }
  if (numLights > BDPT_MAX_LIGHTS) {
    fail(c, "set_lights: more than BDPT_MAX_LIGHTS lights");
    return BDPT_E_LIMIT;
  }
  if (numLights != c->S.numLights) {
    fail(c, "set_lights: the light count differs from the scene's");
    return BDPT_E_INVALID;
  }
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = orderAfterLast(c, st)) return rc;
  const void* arrays[1] = {lights};
  const size_t bytes[1] = {sizeof(bdpt_light) * numLights};
  float* dst[1] = {reinterpret_cast<float*>(const_cast<SceneConst*>(c->S.sc)->lights)};
  if (int rc = stageHostArrays(c, arrays, bytes, 1, dst, st)) return rc;
  retraceLightMaps(c, st);
  HIPCHK(c, hipGetLastError());
  c->hintCamValid = false;
  c->lastStream = st;
  return BDPT_OK;
}

int bdpt_get_refit_info(bdpt_ctx* c, bdpt_refit_info* out) {
  if (!c || !out) return BDPT_E_INVALID;
  if (!c->haveScene) return BDPT_E_STATE;
  ENTER(c);
  *out = bdpt_refit_info{};
  out->sahCostBuilt = c->bvhInfo.sahCost;
  out->sahCost = c->bvhInfo.sahCost;
  out->numUpdates = c->numUpdates;
  if (c->numUpdates == 0) return BDPT_OK;
  HIPCHK(c, hipDeviceSynchronize());
  std::vector<float> area((size_t)c->refit.numNodes * 4);
  float root[6] = {0, 0, 0, 0, 0, 0};
  if (c->refit.numNodes) {
    HIPCHK(c, hipMemcpy(area.data(), c->refit.childArea, area.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(root, c->refit.box, sizeof(root), hipMemcpyDeviceToHost));
  }
  out->sahCost = bvhRefitSah(c->refitPlan, root, area.data());
  return BDPT_OK;
}

// Test hook: FNV-1a over the context's records as they stand (synchronises)
int bdpt_ctx_recs_hash(bdpt_ctx* c, uint64_t* out_hash) {
  if (!c || !out_hash) return BDPT_E_INVALID;
  if (!c->haveScene) return BDPT_E_STATE;
  ENTER(c);
  HIPCHK(c, hipDeviceSynchronize());
  std::vector<BvhRec> recs(c->S.numRecs);
  HIPCHK(c, hipMemcpy(recs.data(), c->S.recs, recs.size() * sizeof(BvhRec), hipMemcpyDeviceToHost));
  uint64_t h = 1469598103934665603ull;
  const uint8_t* b = reinterpret_cast<const uint8_t*>(recs.data());
  for (size_t i = 0; i < recs.size() * sizeof(BvhRec); i++) h = (h ^ b[i]) * 1099511628211ull;
  *out_hash = h;
  return BDPT_OK;
}

namespace {
int resizeRows(bdpt_ctx* c, uint32_t width, uint32_t height, uint32_t maxDepth);
}

int bdpt_resize(bdpt_ctx* c, uint32_t width, uint32_t height, bdpt_tile tile, uint32_t maxDepth) {
  if (!c) return BDPT_E_INVALID;
  if (!width || !height || tile.y0 > tile.y1 || tile.y1 > height) {
    fail(c, "resize: bad frame or tile");
    return BDPT_E_INVALID;
  }
  c->rowRanges.clear();
  if (tile.y1 > tile.y0) c->rowRanges.push_back({tile.y0, tile.y1});
  c->tileRows = tile.y1 - tile.y0;
  c->stripes = bdpt_stripes{0, 1, 0};
  c->sl = SplatLayout{1, 1, height};  // frame order
  return resizeRows(c, width, height, maxDepth);
}

// Interleaved stripes: rows are dealt to `numOwners` contexts in stripes of `stripeRows`; this one
// renders the stripes s with s % numOwners == owner.  The splat buffer becomes owner-major (bdpt_get_tile_info).
int bdpt_resize_stripes(bdpt_ctx* c, uint32_t width, uint32_t height, bdpt_stripes st, uint32_t maxDepth) {
  if (!c) return BDPT_E_INVALID;
  if (!width || !height || !st.stripeRows || !st.numOwners || st.owner >= st.numOwners) {
    fail(c, "resize_stripes: bad frame or stripe description");
    return BDPT_E_INVALID;
  }
  c->rowRanges.clear();
  c->tileRows = 0;
  const uint32_t numStripes = (height + st.stripeRows - 1) / st.stripeRows;
  for (uint32_t s = st.owner; s < numStripes; s += st.numOwners) {
    const uint32_t a = s * st.stripeRows, b = std::min(height, a + st.stripeRows);
    c->rowRanges.push_back({a, b});
    c->tileRows += b - a;
  }
  c->stripes = st;
  c->sl = SplatLayout{st.stripeRows, st.numOwners, ((numStripes + st.numOwners - 1) / st.numOwners) * st.stripeRows};
  return resizeRows(c, width, height, maxDepth);
}

uint32_t bdpt_stripe_rows(uint32_t height, uint32_t numOwners) {
  const uint32_t per = height / std::max(1u, numOwners * 4u);
  return std::max(1u, std::min(8u, per));
}
int bdpt_get_tile_info(const bdpt_ctx* c, bdpt_tile_info* out) {
  if (!c || !out) return BDPT_E_INVALID;
  if (!c->haveSize) return BDPT_E_STATE;
  out->numRows = c->tileRows;
  out->numPixels = c->P.Np;
  out->chunkRows = c->sl.chunkRows;
  out->numRowRanges = (uint32_t)c->rowRanges.size();
  out->splatU64 = (uint64_t)c->sl.owners * c->sl.chunkRows * c->W * 4;
  out->chunkU64 = (uint64_t)c->sl.chunkRows * c->W * 4;
  return BDPT_OK;
}

int bdpt_tile_row_ranges(const bdpt_ctx* c, uint32_t* out_first_last, uint32_t cap) {
  if (!c || !out_first_last) return BDPT_E_INVALID;
  if (!c->haveSize) return BDPT_E_STATE;
  const uint32_t n = std::min<uint32_t>(cap, (uint32_t)c->rowRanges.size());
  for (uint32_t i = 0; i < n; i++) {
    out_first_last[2 * i] = c->rowRanges[i].first;
    out_first_last[2 * i + 1] = c->rowRanges[i].second;
  }
  return (int)n;
}

namespace {
int resizeRows(bdpt_ctx* c, uint32_t width, uint32_t height, uint32_t maxDepth) {
  if (maxDepth > BDPT_MAX_DEPTH) {
    fail(c, "resize: maxDepth exceeds BDPT_MAX_DEPTH");
    return BDPT_E_LIMIT;
  }
  if ((uint64_t)width * height >= (1ull << 32) || (uint64_t)c->sl.owners * c->sl.chunkRows * width >= (1ull << 32)) {
    fail(c, "resize: frame too large");
    return BDPT_E_LIMIT;
  }
  if ((uint64_t)c->tileRows * width >= (1ull << 24)) {
    fail(c, "resize: a tile holds at most 2^24 - 1 pixels (path ids pack the pixel in 24 bits); render in smaller tiles");
    return BDPT_E_LIMIT;
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  freePool(c->frameAllocs);
  freeLightGroups(c);
  freeBmfrHistory(c->bmfr);
  freeBmfrHistory(c->bmfrPlanes);
  c->ownGb = bdpt_gbuffer{};
  c->haveSize = false;
  c->W = width;
  c->H = height;
  c->maxDepth = maxDepth;
  PathBuf P{};
  P.Np = c->tileRows * width;
  P.D1 = std::max<uint32_t>(maxDepth, 1) + 1;
  const size_t np = std::max<uint32_t>(P.Np, 1);
  int rc;
  {
    std::vector<uint32_t> pix;
    pix.reserve(np);
    for (const auto& rr : c->rowRanges)
      for (uint32_t y = rr.first; y < rr.second; y++)
        for (uint32_t x = 0; x < width; x++) pix.push_back(y * width + x);
    if ((rc = devUpload(c, c->frameAllocs, &P.pix, pix.data(), pix.size()))) return rc;
  }
  if ((rc = devAlloc(c, c->frameAllocs, &P.v, (size_t)2 * P.D1 * NF4 * 4 * np))) return rc;
  if ((rc = devAlloc(c, c->frameAllocs, &P.rayDir, (size_t)6 * np))) return rc;
  if ((rc = devAlloc(c, c->frameAllocs, &P.seedL, np))) return rc;
  if ((rc = devAlloc(c, c->frameAllocs, &P.eyeLast, np))) return rc;
  if ((rc = devAlloc(c, c->frameAllocs, &P.lightLast, np))) return rc;
  if ((rc = devAlloc(c, c->frameAllocs, &P.lightReal, np))) return rc;
  // a path queue = kNumSubQueues lists; workgroup b appends to list b % kNumSubQueues
  // (+ one workgroup's worth of slack)
  P.pathSubCap = (uint32_t)((((uint64_t)wavesFor(np) + kNumSubQueues - 1) / kNumSubQueues + 1) * kWave);
  const size_t qcap = (size_t)P.pathSubCap * kNumSubQueues;
  for (int q = 0; q < 3; q++)
    if ((rc = devAlloc(c, c->frameAllocs, &P.queue[q], qcap))) return rc;
  if ((rc = devAlloc(c, c->frameAllocs, &P.qcount, (size_t)kCursorWords))) return rc;
  P.qhead = P.qcount + kCountBlocks * kCursorBlock;
  P.lazyCount = P.qhead + kHeadBlocks * kCursorBlock;
  P.rayCount = P.lazyCount + kLazyBlocks * kCursorBlock;
  P.rayHead = P.rayCount + 2 * kRayCursorBlock;
  {
    // one shadow ray per NEE term, per splat term and per defined connection pair, at most
    const uint32_t D = std::max<uint32_t>(maxDepth, 1);
    const uint64_t slots = (uint64_t)2 * D + numConnectPairs(D);
    // workgroup b appends to sub-queue b % kNumSubQueues: size each for the workgroups it serves
    const uint64_t blocks = wavesFor(np);
    // Producer workgroup b appends to ray sub-queue b % kNumRaySubQueues.  Generators run G lanes per pixel (8, or 16
    // when the context is sized for depth > 8: G x queueGrid workgroups of 64 / G pixels), lazy_gen one lane per pixel:
    // size every sub-queue for the workgroups it can serve under either launch shape.
    const uint64_t queueGridBlocks = (uint64_t)(P.pathSubCap / kWave) * kNumSubQueues;
    const uint64_t pairs = std::max<uint32_t>(numConnectPairs(D), 1);
    uint64_t subCapTerms = 0, subCapPairs = ((queueGridBlocks + kNumRaySubQueues - 1) / kNumRaySubQueues) * kWave * pairs;
    {
      const uint64_t G = D > 8 ? 16 : 8;
      const uint64_t perSub = (queueGridBlocks * G + kNumRaySubQueues - 1) / kNumRaySubQueues;  // workgroups per sub-queue
      subCapTerms = std::max<uint64_t>(subCapTerms, perSub * kWave * 2);                           // one NEE + one splat ray per lane
      subCapPairs = std::max<uint64_t>(subCapPairs, perSub * (kWave / G) * pairs);
    }
    (void)blocks;
    const uint64_t cap = (subCapTerms + subCapPairs) * kNumRaySubQueues;
    if (cap >= (1ull << 32) - 1) {
      fail(c, "resize: shadow-ray queue would exceed 2^32 entries; render in smaller tiles");
      return BDPT_E_LIMIT;
    }
    P.raySubCap[RAY_TERMS] = (uint32_t)subCapTerms;
    P.raySubCap[RAY_PAIRS] = (uint32_t)subCapPairs;
    P.rayBase[RAY_TERMS] = 0;
    P.rayBase[RAY_PAIRS] = (uint32_t)(subCapTerms * kNumRaySubQueues);
    P.rayCap = (uint32_t)cap;
    if ((rc = devAlloc(c, c->frameAllocs, &P.rayQ, (size_t)7 * cap))) return rc;
    if ((rc = devAlloc(c, c->frameAllocs, &P.rayContrib, (size_t)3 * cap))) return rc;
    if ((rc = devAlloc(c, c->frameAllocs, &P.rayVis, (size_t)cap))) return rc;
    if ((rc = devAlloc(c, c->frameAllocs, &P.slotRay, (size_t)slots * np))) return rc;
    if ((rc = devAlloc(c, c->frameAllocs, &P.splatPix, (size_t)D * np))) return rc;
    // Lazy rounds: each costs three small launches, so small tiles (multi-GPU bands) take fewer, larger ones.
    // Lazy rounds: each costs three small launches and cannot finish faster than its slowest ray, so there are few:
    // two or three rounds of kLazyBatchDiv-th shares, the last of which takes every candidate that is left.
    c->lazyRounds = np >= (1u << 18) ? 3 : 2;
    if (const char* e = std::getenv("BDPT_LAZY_ROUNDS")) {  // measurement knob (tools/prof_tile.sh): 1 .. kMaxLazyRounds
      const int v = std::atoi(e);
      if (v >= 1 && v <= kMaxLazyRounds) c->lazyRounds = v;
    }
    // the largest batch any round can ask for: the last round of the front-loaded schedule takes what is left
    const uint32_t batch = numConnectPairs(D);
    if ((rc = devAlloc(c, c->frameAllocs, &P.misE, (size_t)(D + 1) * np))) return rc;
    if ((rc = devAlloc(c, c->frameAllocs, &P.misL, (size_t)(D + 1) * np))) return rc;
    if ((rc = devAlloc(c, c->frameAllocs, &P.lazyCursor, np))) return rc;
    if ((rc = devAlloc(c, c->frameAllocs, &P.lazyRay, (size_t)std::max<uint32_t>(batch, 1) * np))) return rc;
  }
  c->hintPix = nullptr;
  c->hintCamValid = false;
  if (std::getenv("BDPT_NO_HINTS") == nullptr) {
    if ((rc = devAlloc(c, c->frameAllocs, &c->hintPix, (size_t)width * height))) return rc;
    HIPCHK(c, hipMemset(c->hintPix, 0xFF, (size_t)width * height * sizeof(uint32_t)));
  }
  const size_t splatU64 = (size_t)c->sl.owners * c->sl.chunkRows * width * 4;
  if ((rc = devAlloc(c, c->frameAllocs, &c->ownSplat, splatU64))) return rc;
  c->splat = c->ownSplat;
  if ((rc = devAlloc(c, c->frameAllocs, &c->counters, 1))) return rc;
  HIPCHK(c, hipMemset(c->splat, 0, splatU64 * sizeof(unsigned long long)));
  HIPCHK(c, hipMemset(c->counters, 0, sizeof(DevCounters)));
  c->P = P;
  if (!c->evCreated) {
    for (int i = 0; i <= kMaxStages; i++) HIPCHK(c, hipEventCreate(&c->ev[i]));
    for (hipEvent_t& e : c->sideEv) HIPCHK(c, hipEventCreate(&e));
    c->evCreated = true;
  }
  c->haveSize = true;
  return BDPT_OK;
}
}  // namespace

namespace {
// bdpt_gbuffer_execute (prevPosition == NULL) and bdpt_gbuffer_execute_motion
int gbufferRun(bdpt_ctx* c, const bdpt_gbuffer_params* gp, const bdpt_gbuffer* out, float* prevPosition, void* stream) {
  if (!out->worldPosition || !out->worldNormal || !out->materialDiffuse || !out->materialSpecRough ||
      !out->materialExtraParams || !out->emissive) {
    fail(c, "gbuffer_execute: all six channels are required");
    return BDPT_E_INVALID;
  }
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  GBufferDev G{};
  G.cam = c->cam;
  G.gp = *gp;
  G.W = c->W;
  G.H = c->H;
  G.Np = c->P.Np;
  G.pix = c->P.pix;
  G.gb = *out;
  G.counters = nullptr;  // primary rays are tallied analytically by bdpt_get_counters (one per tile pixel)
  G.hintPix = c->hintPix;
  if (c->hintPix && c->tileRows != c->H && (!c->hintCamValid || std::memcmp(&c->hintCam, &c->cam, sizeof(bdpt_camera)) != 0)) {
    GBufferDev A = G;
    A.Np = c->W * c->H;
    A.pix = nullptr;
    launchHintFill(c->S, A, st);
    c->hintCam = c->cam;
    c->hintCamValid = true;
  }
  if (prevPosition) {
    MotionDev M{};
    M.prevPose = c->prevPose;
    M.prevPosition = reinterpret_cast<float4*>(prevPosition);
    launchGBufferMotion(c->S, G, M, st);
  } else {
    launchGBuffer(c->S, G, st);
  }
  HIPCHK(c, hipGetLastError());
  c->lastStream = st;
  return BDPT_OK;
}
}  // namespace

int bdpt_gbuffer_execute(bdpt_ctx* c, const bdpt_gbuffer_params* gp, const bdpt_gbuffer* out, void* stream) {
  if (!c || !gp || !out) return BDPT_E_INVALID;
  if (!c->haveScene || !c->haveCamera || !c->haveSize) {
    fail(c, "gbuffer_execute: scene, camera and size must be set first");
    return BDPT_E_STATE;
  }
  return gbufferRun(c, gp, out, nullptr, stream);
}

// ---- motion: the previous pose (motion.hip) and the calls that read it ----
namespace {
int allocPrevPose(bdpt_ctx* c) {
  if (c->prevPose) return BDPT_OK;
  if (streamIsCapturing(c->lastStream)) {
    fail(c, "prepare: BDPT_PREPARE_MOTION allocates and synchronises: not inside a stream capture");
    return BDPT_E_STATE;
  }
  float4* pose = nullptr;
  if (int rc = devAlloc(c, c->sceneAllocs, &pose, (size_t)c->numTriangles * 3)) return rc;
  HIPCHK(c, hipDeviceSynchronize());  // (updates in flight on any stream: the first previous pose is the current one)
  launchKeepPose(c->S.shade, c->numTriangles, pose, nullptr);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipDeviceSynchronize());
  c->prevPose = pose;
  return BDPT_OK;
}
}  // namespace

int bdpt_keep_pose(bdpt_ctx* c, void* stream) {
  if (!c) return BDPT_E_INVALID;
  if (!c->haveScene || !c->prevPose) {
    fail(c, c->haveScene ? "keep_pose: no previous pose (bdpt_prepare(BDPT_PREPARE_MOTION) first)" : "keep_pose: no scene (bdpt_set_scene first)");
    return BDPT_E_STATE;
  }
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = orderAfterLast(c, st)) return rc;
  launchKeepPose(c->S.shade, c->numTriangles, c->prevPose, st);
  HIPCHK(c, hipGetLastError());
  c->lastStream = st;
  return BDPT_OK;
}

int bdpt_gbuffer_execute_motion(bdpt_ctx* c, const bdpt_gbuffer_params* gp, const bdpt_gbuffer* out, float* prevPosition, void* stream) {
  if (!c || !gp || !out) return BDPT_E_INVALID;
  if (!c->haveScene || !c->haveCamera || !c->haveSize) {
    fail(c, "gbuffer_execute_motion: scene, camera and size must be set first");
    return BDPT_E_STATE;
  }
  if (!c->prevPose) {
    fail(c, "gbuffer_execute_motion: no previous pose (bdpt_prepare(BDPT_PREPARE_MOTION) first)");
    return BDPT_E_STATE;
  }
  if (!aligned(prevPosition, 16)) {
    fail(c, "gbuffer_execute_motion: prevPosition missing or not 16-byte aligned");
    return BDPT_E_INVALID;
  }
  return gbufferRun(c, gp, out, prevPosition, stream);
}

namespace {
// argument checks shared by bdpt_execute and bdpt_execute_tail, and the per-frame constants the kernels take
int frameSetup(bdpt_ctx* c, const bdpt_params* p, const bdpt_gbuffer* in, float* out, hipStream_t st, FrameDev& F) {
  if (!c || !p || !out) return BDPT_E_INVALID;
  ENTER(c);
  if (!in) {  // the context's own channels: the primary stage runs inside bdpt_execute
    if (!c->haveSize) {
      fail(c, "execute: scene, camera and size must be set first");
      return BDPT_E_STATE;
    }
    if (!c->ownGb.worldPosition) {  // bdpt_prepare(BDPT_PREPARE_PRIMARY) was not called: allocate now, unless capturing
      if (streamIsCapturing(st)) {
        fail(c, "execute: the built-in primary stage needs bdpt_prepare(BDPT_PREPARE_PRIMARY) before stream capture");
        return BDPT_E_STATE;
      }
      if (int rc = allocOwnGbuffer(c)) return rc;
    }
    in = &c->ownGb;
  }
  if (!c->haveScene || !c->haveCamera || !c->haveSize) {
    fail(c, "execute: scene, camera and size must be set first");
    return BDPT_E_STATE;
  }
  if (p->maxDepth > c->maxDepth) {
    fail(c, "execute: params.maxDepth exceeds the depth given to bdpt_resize");
    return BDPT_E_LIMIT;
  }
  if (p->matIndex > 1) {
    fail(c, "execute: matIndex must be 0 (GGX) or 1 (Lambertian)");
    return BDPT_E_INVALID;
  }
  if (!in->worldPosition || !in->worldNormal || !in->materialDiffuse || !in->materialSpecRough || !in->emissive) {
    fail(c, "execute: G-buffer channels missing");
    return BDPT_E_INVALID;
  }
  F = FrameDev{};
  F.cam = c->cam;
  F.p = *p;
  F.W = c->W;
  F.H = c->H;
  F.sl = c->sl;
  F.out = out;
  F.splat = c->splat;
  F.gb = *in;
  F.counters = c->counters;  // ray tallies are always on; node/triangle visits need BDPT_PARAM_COUNTERS
  F.envMap = c->env.envMap;
  F.envW = c->env.width;
  F.envH = c->env.height;
  for (int k = 0; k < 3; k++) F.envColor[k] = c->env.color[k];
  F.hintPix = c->hintPix;
  return BDPT_OK;
}

// Connection pairs whose contribution is exactly zero, for the pixels no visible connection has saturated
// yet (DESIGN.md "Lazy connection rounds"), then the splat fold-in unless the caller defers it.
// V: the frame's variant (FrameVariant), for the lazy check and the resolve.
int connectionTail(bdpt_ctx* c, const FrameDev& F, hipStream_t st, const FrameVariant& V) {
  const PathBuf& P = c->P;
  const bdpt_params* p = &F.p;
  const int D = (int)p->maxDepth;
  if (!(p->flags & BDPT_PARAM_NO_CONNECT) && D >= 2) {
    const int nPairs = (int)numConnectPairs((uint32_t)D);
    // Schedule: rounds of ceil(pairs / kLazyBatchDiv) candidates; the last round takes everything that is left.  A launch
    // cannot finish faster than its slowest ray (~0.1 ms), so once few pixels are pending one big round beats several.
    // (Front rounds of 1,2,4 / 2,4 / 1,4 / 2,6 / 3 / 1,2,4,8 / 2 candidates were measured within 5 % of this one:
    // most lazy rays belong to pixels whose candidates are all occluded.  profiles/README.md)
    const int b0 = (nPairs + kLazyBatchDiv - 1) / kLazyBatchDiv;
    int left = nPairs;
    for (int r = 0; r < c->lazyRounds && left > 0; r++) {
      const int batch = (r + 1 == c->lazyRounds) ? left : (b0 < left ? b0 : left);
      left -= batch;
      uint32_t* list = P.queue[1 + (r & 1)];
      uint32_t* next = P.queue[1 + ((r + 1) & 1)];
      HIPCHK(c, hipMemsetAsync(P.rayCount + (size_t)RAY_PAIRS * kRayCursorBlock, 0, kRayCursorBlock * sizeof(uint32_t), st));
      HIPCHK(c, hipMemsetAsync(P.rayHead + (size_t)RAY_PAIRS * kRayCursorBlock, 0, kRayCursorBlock * sizeof(uint32_t), st));
      launchLazyGen(F, P, list, P.lazyCount + (size_t)r * kCursorBlock, batch, st);
      stageMark(c, st, "lazy_gen");
      launchTraceShadow(c->S, F, P, RAY_PAIRS, c->grids, c->numCUs, st);
      stageMark(c, st, "lazy_trace");
      launchLazyCheck(F, P, V, list, P.lazyCount + (size_t)r * kCursorBlock, batch, next, P.lazyCount + (size_t)(r + 1) * kCursorBlock,
                      st);
    }
    stageMark(c, st, "lazy_check");
  }
  if (!(p->flags & BDPT_PARAM_DEFER_RESOLVE)) {  // (refused for group and masked frames)
    launchFrameResolve(F, P, V, st);
    stageMark(c, st, V.kind == FrameKind::Groups ? "resolve_groups" : V.kind == FrameKind::Masked ? "resolve_masked" : "resolve");
  }
  HIPCHK(c, hipGetLastError());
  c->lastStream = st;
  return BDPT_OK;
}
}  // namespace

namespace {
// bdpt_execute, bdpt_execute_light_groups and bdpt_execute_masked: the same stages and the same rays.  The per-pixel
// stages take the variant V; a group frame also clears its splat-value planes, and a masked frame runs the generators of
// eye-side terms (NEE, connections) over its eye list (`PE`: the PathBuf with the eye list as its pixel list).
// groupsTakeArea: a group frame whose caller assigned the emitter table a group (bdpt_execute_grouped)
int executeFrame(bdpt_ctx* c, const bdpt_params* p, const bdpt_gbuffer* in, float* out, void* stream, const FrameVariant& V0,
                 bool groupsTakeArea = false) {
  FrameDev F;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = frameSetup(c, p, in, out, st, F)) return rc;
  FrameVariant V = V0;
  if (p->flags & BDPT_PARAM_AREA_LIGHTS) {
    // (the pdf an area-light vertex needs in the MIS prefix is a design question of its own; the planes of
    // bdpt_execute_light_groups have no slot for the table: bdpt_execute_grouped assigns it one)
    if (p->flags & (BDPT_PARAM_MIS_POWER | BDPT_PARAM_MIS_LINEAR)) {
      fail(c, "execute: BDPT_PARAM_AREA_LIGHTS is not supported with BDPT_PARAM_MIS_POWER / _LINEAR");
      return BDPT_E_INVALID;
    }
    if (V.kind == FrameKind::Groups && !groupsTakeArea) {
      fail(c, "light groups: BDPT_PARAM_AREA_LIGHTS is not supported (the group planes have no slot for area lights)");
      return BDPT_E_INVALID;
    }
    if (int rc = ensureAreaLights(c, st)) return rc;
    V.area = c->area;  // n == 0 (no emitter): the plain instances
    if (V.kind == FrameKind::Groups && V.area.n) V.groups.areaW = V.area.total;
  }
  const PathBuf& P = c->P;
  PathBuf PE = P;
  if (V.kind == FrameKind::Masked) {
    PE.queue[0] = V.mask.eye;
    PE.qcount = V.mask.eyeCount;
  }
  if (!in) {
    // Built-in primary stage: pinhole camera, this frame's jitter and counter, the default constant
    // environment (SharedUtils/ResourceManager.cpp:77-87) — what LightProbeGBufferPass does with its defaults.
    bdpt_gbuffer_params gp{};
    gp.pixelJitter[0] = p->pixelJitter[0];
    gp.pixelJitter[1] = p->pixelJitter[1];
    gp.focalLen = 1.0f;
    gp.frameCount = p->frameCount;
    gp.envColor[0] = gp.envColor[1] = 0.5f;
    gp.envColor[2] = 0.8f;
    gp.envColor[3] = 1.0f;
    if (int rc = bdpt_gbuffer_execute(c, &gp, &c->ownGb, stream)) return rc;
  }

  c->numStages = 0;
  c->numSideStages = 0;
  if (c->timing) HIPCHK(c, hipEventRecord(c->ev[0], st));
  HIPCHK(c, hipMemsetAsync(P.qcount, 0, (size_t)kCursorWords * sizeof(uint32_t), st));
  HIPCHK(c, hipMemsetAsync(c->splat, 0, (size_t)c->sl.owners * c->sl.chunkRows * c->W * 4 * sizeof(unsigned long long), st));
  if (V.kind == FrameKind::Groups)
    HIPCHK(c, hipMemsetAsync(V.groups.splat, 0, (size_t)V.groups.numGroups * V.groups.framePix * 4 * sizeof(unsigned long long), st));
  if (!(p->flags & BDPT_PARAM_KEEP_COUNTERS)) HIPCHK(c, hipMemsetAsync(c->counters, 0, sizeof(DevCounters), st));
  stageMark(c, st, "clear");

  launchInitPaths(c->S, F, P, V, st);
  stageMark(c, st, "init_paths");

  // Both walks (eye vertices 2..D, BDPTMain.rt.hlsl:106-112; light vertices 1..D, :138-145) in one persistent
  // launch: traversal and hit/miss shading alternate inside the kernel, lanes re-arm themselves per bounce.
  launchWalk(c->S, F, P, V, c->grids, c->numCUs, st);
  stageMark(c, st, "walk");

  // NEE terms (caller's stream) and splat terms (second stream) are generated side by side and traced at once (ray
  // class RAY_TERMS) while the connection generator — the long one — fills the RAY_PAIRS queue on the second stream;
  // the connection rays are traced when both are done.  (The MIS weights read both paths: everything sequential then.)
  const bool mis = (p->flags & (BDPT_PARAM_MIS_POWER | BDPT_PARAM_MIS_LINEAR)) != 0;
  if (mis) {
    launchMisPrefix(F, P, st);
    stageMark(c, st, "mis_prefix");
    launchGenNee(c->S, F, PE, V.area, st);
    stageMark(c, st, "gen_nee");
    launchGenSplat(c->S, F, P, st);
    stageMark(c, st, "gen_splat");
    launchGenConnect(c->S, F, PE, st);
    stageMark(c, st, "gen_connect");
    launchTraceShadow(c->S, F, P, RAY_TERMS, c->grids, c->numCUs, st);
    stageMark(c, st, "trace_terms");
  } else {
    // Stage names: a stage of the caller's stream is ONE kernel (or one memset group) — "gen_nee", "trace_terms",
    // "trace_pairs" ... — or a wait for the second stream ("splat_wait", "connect_wait": what of gen_splat / gen_connect
    // the caller's stream did not cover); the second stream's kernels are timed by event pairs of their own and reported
    // behind the caller's stages as "side:gen_splat", "side:gen_connect" (they overlap the stages above: not part of the
    // critical-path sum).
    HIPCHK(c, hipEventRecord(c->evFork, st));
    HIPCHK(c, hipStreamWaitEvent(c->walkStream, c->evFork, 0));
    sideBegin(c, c->walkStream, "side:gen_splat");
    launchGenSplat(c->S, F, P, c->walkStream);  // beside the NEE generator; both are short and latency-bound
    sideEnd(c, c->walkStream);
    HIPCHK(c, hipEventRecord(c->evSplat, c->walkStream));
    sideBegin(c, c->walkStream, "side:gen_connect");
    launchGenConnect(c->S, F, PE, c->walkStream);
    sideEnd(c, c->walkStream);
    HIPCHK(c, hipEventRecord(c->evJoin, c->walkStream));
    launchGenNee(c->S, F, PE, V.area, st);
    stageMark(c, st, "gen_nee");
    HIPCHK(c, hipStreamWaitEvent(st, c->evSplat, 0));
    stageMark(c, st, "splat_wait");
    launchTraceShadow(c->S, F, P, RAY_TERMS, c->grids, c->numCUs, st);
    stageMark(c, st, "trace_terms");
    HIPCHK(c, hipStreamWaitEvent(st, c->evJoin, 0));
    stageMark(c, st, "connect_wait");
  }
  launchTraceShadow(c->S, F, P, RAY_PAIRS, c->grids, c->numCUs, st);
  stageMark(c, st, "trace_pairs");
  launchGather(F, P, V, P.queue[1], P.lazyCount, st);
  stageMark(c, st, "gather");
  // Everything that touches the splat buffer is enqueued by now: a tiled host may start its exchange here
  // and run the connection tail beside it (BDPT_PARAM_DEFER_TAIL + bdpt_execute_tail).
  if (p->flags & BDPT_PARAM_DEFER_TAIL) {
    HIPCHK(c, hipGetLastError());
    c->lastStream = st;
    return BDPT_OK;
  }
  return connectionTail(c, F, st, V);
}

// the group path's buffers, with at least `planes` splat-value planes; not while the stream is being captured
int allocLightGroups(bdpt_ctx* c, hipStream_t st, uint32_t planes) {
  if (c->groupSplat && c->groupSplatPlanes >= planes) return BDPT_OK;
  if (streamIsCapturing(st)) {
    fail(c, "light groups: the splat planes need bdpt_prepare(BDPT_PREPARE_LIGHT_GROUPS / _LIGHT_GROUP_TABLE) before stream capture");
    return BDPT_E_STATE;
  }
  if (c->groupSplat) {  // too few planes for this assignment: frames in flight still use them
    HIPCHK(c, hipDeviceSynchronize());
    freeLightGroups(c);
  }
  const size_t n = (size_t)c->W * c->H;
  void *sp = nullptr, *li = nullptr;
  if (hipMalloc(&sp, std::max<size_t>((size_t)planes * n * 4 * sizeof(unsigned long long), 16)) != hipSuccess ||
      hipMalloc(&li, std::max<size_t>(c->P.Np, 16)) != hipSuccess) {
    if (sp) (void)hipFree(sp);
    fail(c, "light groups: hipMalloc of the splat planes failed");
    return BDPT_E_NOMEM;
  }
  c->groupSplat = reinterpret_cast<unsigned long long*>(sp);
  c->groupSplatPlanes = planes;
  c->groupLightIdx = reinterpret_cast<uint8_t*>(li);
  return BDPT_OK;
}

// What bdpt_execute_light_groups, bdpt_execute_masked and the adaptive calls refuse alike, as "<what>: ...": the deferred
// stages (when params are given), a context without scene or size, and one that does not render the whole frame.
int wholeFrameCheck(bdpt_ctx* c, const bdpt_params* p, const std::string& what) {
  if (p && (p->flags & (BDPT_PARAM_DEFER_RESOLVE | BDPT_PARAM_DEFER_TAIL))) {
    fail(c, what + ": BDPT_PARAM_DEFER_RESOLVE and BDPT_PARAM_DEFER_TAIL are not supported");
    return BDPT_E_INVALID;
  }
  if (!c->haveScene || !c->haveSize) {
    fail(c, what + ": scene and size must be set first");
    return BDPT_E_STATE;
  }
  if (c->stripes.stripeRows != 0 || c->tileRows != c->H) {
    fail(c, what + ": the context must render the whole frame (no tile, no stripes)");
    return BDPT_E_INVALID;
  }
  return BDPT_OK;
}
}  // namespace

int bdpt_execute(bdpt_ctx* c, const bdpt_params* p, const bdpt_gbuffer* in, float* out, void* stream) {
  return executeFrame(c, p, in, out, stream, FrameVariant{});
}

int bdpt_execute_light_groups(bdpt_ctx* c, const bdpt_params* p, const bdpt_gbuffer* in, float* out, float* groups, void* stream) {
  if (!c) return BDPT_E_INVALID;
  if (!groups) {
    fail(c, "light groups: groups is NULL");
    return BDPT_E_INVALID;
  }
  if (int rc = wholeFrameCheck(c, p, "light groups")) return rc;
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = allocLightGroups(c, st, c->S.numLights)) return rc;
  FrameVariant V;  // the identity assignment: group k = light k
  V.kind = FrameKind::Groups;
  V.groups.planes = groups;
  V.groups.splat = c->groupSplat;
  V.groups.lightIdx = c->groupLightIdx;
  V.groups.numLights = c->S.numLights;
  V.groups.numGroups = c->S.numLights;
  V.groups.framePix = (uint64_t)c->W * c->H;
  for (uint32_t i = 0; i < c->S.numLights; i++) V.groups.groupOf[i] = (uint8_t)i;
  return executeFrame(c, p, in, out, stream, V);
}

int bdpt_execute_grouped(bdpt_ctx* c, const bdpt_params* p, const bdpt_gbuffer* in, float* out, const bdpt_light_group_desc* d,
                         void* stream) {
  if (!c) return BDPT_E_INVALID;
  if (!p || !out) {
    fail(c, "execute_grouped: params or out is NULL");
    return BDPT_E_INVALID;
  }
  if (!d || !d->planes || !d->groupOf) {
    fail(c, "execute_grouped: the descriptor, its planes or its groupOf is NULL");
    return BDPT_E_INVALID;
  }
  if (int rc = wholeFrameCheck(c, p, "execute_grouped")) return rc;
  if (d->numGroups < 1 || d->numGroups > BDPT_MAX_LIGHTS + 1) {
    fail(c, "execute_grouped: numGroups must be 1 .. BDPT_MAX_LIGHTS + 1");
    return BDPT_E_INVALID;
  }
  const bool area = (p->flags & BDPT_PARAM_AREA_LIGHTS) != 0;
  const uint32_t numLights = c->S.numLights;
  if (d->numAssigned != numLights + (area ? 1u : 0u)) {
    fail(c, "execute_grouped: numAssigned must be numLights, or numLights + 1 with BDPT_PARAM_AREA_LIGHTS");
    return BDPT_E_INVALID;
  }
  for (uint32_t i = 0; i < d->numAssigned; i++)
    if (d->groupOf[i] >= d->numGroups) {
      fail(c, "execute_grouped: groupOf[" + std::to_string(i) + "] is not below numGroups");
      return BDPT_E_INVALID;
    }
  if (d->reserved[0] || d->reserved[1]) {
    fail(c, "execute_grouped: reserved must be 0");
    return BDPT_E_INVALID;
  }
  if (area && (p->flags & (BDPT_PARAM_MIS_POWER | BDPT_PARAM_MIS_LINEAR))) {  // (before anything is allocated)
    fail(c, "execute: BDPT_PARAM_AREA_LIGHTS is not supported with BDPT_PARAM_MIS_POWER / _LINEAR");
    return BDPT_E_INVALID;
  }
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = allocLightGroups(c, st, d->numGroups)) return rc;
  FrameVariant V;
  V.kind = FrameKind::Groups;
  V.groups.planes = d->planes;
  V.groups.splat = c->groupSplat;
  V.groups.lightIdx = c->groupLightIdx;
  V.groups.numLights = numLights;
  V.groups.numGroups = d->numGroups;
  V.groups.framePix = (uint64_t)c->W * c->H;
  for (uint32_t i = 0; i < d->numAssigned; i++) V.groups.groupOf[i] = d->groupOf[i];
  return executeFrame(c, p, in, out, stream, V, true);
}

int bdpt_execute_masked(bdpt_ctx* c, const bdpt_params* p, const bdpt_gbuffer* in, const uint8_t* mask, float* out, void* stream) {
  if (!c) return BDPT_E_INVALID;
  if (!mask) {
    fail(c, "execute_masked: mask is NULL");
    return BDPT_E_INVALID;
  }
  if (int rc = wholeFrameCheck(c, p, "execute_masked")) return rc;
  // The eye list: the active valid pixels, which init_paths pushes (where it lives: kEyeCountBlock).  Under MIS the walk's
  // eye lists stay the valid list: every valid pixel's eye prefix products are read by its splats.
  const PathBuf& P = c->P;
  const bool misOn = p && (p->flags & (BDPT_PARAM_MIS_POWER | BDPT_PARAM_MIS_LINEAR)) != 0;
  FrameVariant V;
  V.kind = FrameKind::Masked;
  V.mask.mask = mask;
  V.mask.eye = P.queue[2];
  V.mask.eyeCount = P.lazyCount + kEyeCountBlock * kCursorBlock;
  V.mask.walkEye = misOn ? P.queue[0] : V.mask.eye;
  V.mask.walkEyeCount = misOn ? P.qcount : V.mask.eyeCount;
  return executeFrame(c, p, in, out, stream, V);
}

namespace {
// the arguments of bdpt_adaptive_reset / _update: a whole-frame context and every state buffer
int adaptiveSetup(bdpt_ctx* c, const bdpt_adaptive_state* s, const char* what, AdaptiveDev& A) {
  if (!s || !s->mean || !s->m2 || !s->count || !s->mask || !s->active) {
    fail(c, std::string(what) + ": a state buffer is NULL");
    return BDPT_E_INVALID;
  }
  if (int rc = wholeFrameCheck(c, nullptr, what)) return rc;
  if (reinterpret_cast<uintptr_t>(s->mean) % 16 != 0) {
    fail(c, std::string(what) + ": mean must be 16-byte aligned (RGBA32F)");
    return BDPT_E_INVALID;
  }
  A = AdaptiveDev{};
  A.mean = reinterpret_cast<float4*>(s->mean);
  A.m2 = s->m2;
  A.count = s->count;
  A.mask = s->mask;
  A.active = s->active;
  A.W = c->W;
  A.H = c->H;
  return BDPT_OK;
}
}  // namespace

int bdpt_adaptive_reset(bdpt_ctx* c, const bdpt_adaptive_state* s, void* stream) {
  if (!c) return BDPT_E_INVALID;
  AdaptiveDev A;
  if (int rc = adaptiveSetup(c, s, "adaptive_reset", A)) return rc;
  ENTER(c);
  launchAdaptiveReset(A, reinterpret_cast<hipStream_t>(stream));
  HIPCHK(c, hipGetLastError());
  return BDPT_OK;
}

int bdpt_adaptive_update(bdpt_ctx* c, const bdpt_adaptive_params* a, const bdpt_adaptive_state* s, float* frame, void* stream) {
  if (!c) return BDPT_E_INVALID;
  if (!a || !frame) {
    fail(c, "adaptive_update: params or frame is NULL");
    return BDPT_E_INVALID;
  }
  const uint32_t b = a->blockSize;
  if (b != 1 && b != 2 && b != 4 && b != 8 && b != 16) {
    fail(c, "adaptive_update: blockSize must be 1, 2, 4, 8 or 16");
    return BDPT_E_INVALID;
  }
  if (a->minSamples < 2 || a->maxSamples < a->minSamples) {
    fail(c, "adaptive_update: need 2 <= minSamples <= maxSamples");
    return BDPT_E_INVALID;
  }
  if (reinterpret_cast<uintptr_t>(frame) % 16 != 0) {
    fail(c, "adaptive_update: frame must be 16-byte aligned (RGBA32F)");
    return BDPT_E_INVALID;
  }
  AdaptiveDev A;
  if (int rc = adaptiveSetup(c, s, "adaptive_update", A)) return rc;
  A.frame = reinterpret_cast<float4*>(frame);
  A.threshold = a->threshold;
  A.epsilon = a->epsilon;
  A.minSamples = a->minSamples;
  A.maxSamples = a->maxSamples;
  A.blockSize = b;
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = orderAfterLast(c, st)) return rc;  // (the sum words: one update of a context at a time)
  launchAdaptiveUpdate(A, c->adaptiveSum, st);
  HIPCHK(c, hipGetLastError());
  c->lastStream = st;
  return BDPT_OK;
}

int bdpt_execute_tail(bdpt_ctx* c, const bdpt_params* p, const bdpt_gbuffer* in, float* out, void* stream) {
  FrameDev F;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = frameSetup(c, p, in, out, st, F)) return rc;
  stageMark(c, st, "tail_wait");  // stream time between the end of phase 1 and this call (the host's exchange set-up), not a kernel
  return connectionTail(c, F, st, FrameVariant{});
}

// Allocate the optional buffers up front so that no later execute allocates (hipGraph capture, latency).
int bdpt_prepare(bdpt_ctx* c, uint32_t what) {
  if (!c) return BDPT_E_INVALID;
  if ((what & ~(BDPT_PREPARE_REFIT | BDPT_PREPARE_AREA_LIGHTS | BDPT_PREPARE_MOTION | BDPT_PREPARE_REFIT_PIECES)) || !what) {
    if (!c->haveSize) {
      fail(c, "prepare: bdpt_resize must be called first");
      return BDPT_E_STATE;
    }
  }
  if ((what & (BDPT_PREPARE_REFIT | BDPT_PREPARE_REFIT_PIECES)) && !c->haveScene) {
    fail(c, "prepare: BDPT_PREPARE_REFIT needs a scene");
    return BDPT_E_STATE;
  }
  if ((what & BDPT_PREPARE_AREA_LIGHTS) && !c->haveScene) {
    fail(c, "prepare: BDPT_PREPARE_AREA_LIGHTS needs a scene");
    return BDPT_E_STATE;
  }
  if ((what & BDPT_PREPARE_MOTION) && !c->haveScene) {
    fail(c, "prepare: BDPT_PREPARE_MOTION needs a scene");
    return BDPT_E_STATE;
  }
  if ((what & (BDPT_PREPARE_LIGHT_GROUPS | BDPT_PREPARE_LIGHT_GROUP_TABLE)) && !c->haveScene) {
    fail(c, "prepare: BDPT_PREPARE_LIGHT_GROUPS needs a scene (the planes are per light)");
    return BDPT_E_STATE;
  }
  ENTER(c);
  if (what & BDPT_PREPARE_REFIT_PIECES) {  // (implies BDPT_PREPARE_REFIT)
    if (int rc = ensureRefitPieces(c)) return rc;
  } else if (what & BDPT_PREPARE_REFIT) {
    if (int rc = ensureRefit(c, nullptr)) return rc;
  }
  if (what & BDPT_PREPARE_PRIMARY)
    if (int rc = allocOwnGbuffer(c)) return rc;
  if (what & BDPT_PREPARE_BMFR)  // (whole-frame history also on a band / stripes context: bdpt_bmfr_execute takes whole-frame buffers)
    if (int rc = ensureBmfrHistory(c, c->bmfr, 1, nullptr, "bmfr", kBmfrPrepare)) return rc;
  if (what & (BDPT_PREPARE_LIGHT_GROUPS | BDPT_PREPARE_LIGHT_GROUP_TABLE))  // (_TABLE: a plane for the emitter table's group too)
    if (int rc = allocLightGroups(c, nullptr, c->S.numLights + ((what & BDPT_PREPARE_LIGHT_GROUP_TABLE) ? 1u : 0u))) return rc;
  if (what & BDPT_PREPARE_AREA_LIGHTS)
    if (int rc = ensureAreaLights(c, nullptr)) return rc;
  if (what & BDPT_PREPARE_MOTION)
    if (int rc = allocPrevPose(c)) return rc;
  return BDPT_OK;
}

// BlockwiseMultiOrderFeatureRegression::execute (DenoisePass.cpp:146-204)
namespace {
// what every denoise entry point checks first
int bmfrCheck(bdpt_ctx* c, const bdpt_gbuffer* g, const char* who) {
  if (!c->haveSize) {
    fail(c, std::string(who) + ": bdpt_resize must be called first");
    return BDPT_E_STATE;
  }
  if (!g->worldPosition || !g->worldNormal || !g->materialDiffuse) {
    fail(c, std::string(who) + ": WorldPosition, WorldNormal and MaterialDiffuse are required");
    return BDPT_E_INVALID;
  }
  return BDPT_OK;
}

// One denoise of `count` images (checked by the entry point; its array is copied here) on history h, which holds at least
// `count` slots: enqueues the pass on st and flips the history.
int bmfrRun(bdpt_ctx* c, BmfrHistory& h, const bdpt_bmfr_params* p, const bdpt_gbuffer* g, const float* prevPosition, float* const* planes,
            uint32_t count, hipStream_t st) {
  const size_t n = (size_t)c->W * c->H;
  BmfrDev A{};
  A.W = c->W;
  A.H = c->H;
  A.frame = p->frameNumber;
  A.full = (p->flags & BDPT_BMFR_FULL_FRAME) ? 1u : 0u;
  A.doPre = (p->flags & BDPT_BMFR_PREPROCESS) ? 1u : 0u;
  for (int k = 0; k < 16; k++) A.m[k] = p->prevViewProj[k];
  A.curPos = reinterpret_cast<const float4*>(g->worldPosition);
  A.curNorm = g->worldNormal;
  A.albedo = g->materialDiffuse;
  const int r = h.read, w = 1 - r;
  A.prevPosR = h.pos[r];
  A.prevNormR = h.norm[r];
  A.prevPosW = h.pos[w];
  A.prevNormW = h.norm[w];
  A.accept = h.accept;
  A.prevPixel = h.prevPixel;
  A.prevPos = reinterpret_cast<const float4*>(prevPosition);
  A.numPlanes = count;
  A.read = (uint32_t)r;
  for (uint32_t k = 0; k < count; k++) A.planes[k] = reinterpret_cast<float4*>(planes[k]);
  A.histNoisy = h.noisy;
  A.histFiltered = h.filtered;
  if (!(p->flags & BDPT_BMFR_POSTPROCESS))  // no new filtered frames this time: the old ones stay on the read side next frame
    for (uint32_t k = 0; k < count; k++)
      HIPCHK(c, hipMemcpyAsync(h.filtered + (2 * (size_t)k + w) * n, h.filtered + (2 * (size_t)k + r) * n, n * sizeof(float4),
                               hipMemcpyDeviceToDevice, st));
  launchBmfr(A, p->flags, st);
  HIPCHK(c, hipGetLastError());
  h.read = w;
  c->lastStream = st;
  return BDPT_OK;
}

// bdpt_bmfr_execute (prevPosition == NULL) and bdpt_bmfr_execute_motion
int bmfrSingle(bdpt_ctx* c, const bdpt_bmfr_params* p, const bdpt_gbuffer* g, const float* prevPosition, float* noisy, void* stream) {
  if (int rc = bmfrCheck(c, g, "bmfr")) return rc;
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = ensureBmfrHistory(c, c->bmfr, 1, st, "bmfr", kBmfrPrepare)) return rc;
  return bmfrRun(c, c->bmfr, p, g, prevPosition, &noisy, 1, st);
}
}  // namespace

int bdpt_bmfr_execute(bdpt_ctx* c, const bdpt_bmfr_params* p, const bdpt_gbuffer* g, float* noisy, void* stream) {
  if (!c || !p || !g || !noisy) return BDPT_E_INVALID;
  return bmfrSingle(c, p, g, nullptr, noisy, stream);
}

int bdpt_bmfr_execute_motion(bdpt_ctx* c, const bdpt_bmfr_params* p, const bdpt_gbuffer* g, const float* prevPosition, float* noisy,
                             void* stream) {
  if (!c || !p || !g || !noisy) return BDPT_E_INVALID;
  if (!aligned(prevPosition, 16)) {
    fail(c, "bmfr_execute_motion: prevPosition missing or not 16-byte aligned");
    return BDPT_E_INVALID;
  }
  return bmfrSingle(c, p, g, prevPosition, noisy, stream);
}

int bdpt_bmfr_reset(bdpt_ctx* c) {
  if (!c) return BDPT_E_INVALID;
  return resetBmfrHistory(c, c->bmfr);
}

// [pos | norm | noisy | filtered] of the read side (slot 0 of the single-image history), W * H float4 each
int bdpt_bmfr_history_bytes(const bdpt_ctx* c, uint64_t* out_bytes) {
  if (!c || !out_bytes) return BDPT_E_INVALID;
  *out_bytes = (c->haveSize && c->bmfr.accept) ? (uint64_t)c->W * c->H * sizeof(float4) * 4 : 0;
  return BDPT_OK;
}
int bdpt_bmfr_save_history(bdpt_ctx* c, void* blob, uint64_t bytes) {
  if (!c || !blob) return BDPT_E_INVALID;
  if (!c->haveSize || !c->bmfr.accept) {
    fail(c, "bmfr_save_history: no history (the denoiser has not run on this context)");
    return BDPT_E_STATE;
  }
  const size_t n = (size_t)c->W * c->H, plane = n * sizeof(float4);
  if (bytes < 4 * plane) return BDPT_E_INVALID;
  ENTER(c);
  HIPCHK(c, hipStreamSynchronize(c->lastStream));
  const BmfrHistory& h = c->bmfr;
  const float4* src[4] = {h.pos[h.read], h.norm[h.read], h.noisy + h.read * n, h.filtered + h.read * n};
  for (int k = 0; k < 4; k++) HIPCHK(c, hipMemcpy(static_cast<uint8_t*>(blob) + k * plane, src[k], plane, hipMemcpyDeviceToHost));
  return BDPT_OK;
}
int bdpt_bmfr_load_history(bdpt_ctx* c, const void* blob, uint64_t bytes) {
  if (!c || !blob) return BDPT_E_INVALID;
  if (!c->haveSize) {
    fail(c, "bmfr_load_history: bdpt_resize must be called first");
    return BDPT_E_STATE;
  }
  const size_t n = (size_t)c->W * c->H, plane = n * sizeof(float4);
  if (bytes != 4 * plane) {
    fail(c, "bmfr_load_history: the blob was written for another frame size");
    return BDPT_E_INVALID;
  }
  ENTER(c);
  if (int rc = ensureBmfrHistory(c, c->bmfr, 1, nullptr, "bmfr", kBmfrPrepare)) return rc;  // (a new one is reset: read side 0)
  HIPCHK(c, hipStreamSynchronize(c->lastStream));
  const BmfrHistory& h = c->bmfr;
  float4* dst[4] = {h.pos[h.read], h.norm[h.read], h.noisy + h.read * n, h.filtered + h.read * n};
  for (int k = 0; k < 4; k++) HIPCHK(c, hipMemcpy(dst[k], static_cast<const uint8_t*>(blob) + k * plane, plane, hipMemcpyHostToDevice));
  return BDPT_OK;
}

// ---- bdpt_bmfr_execute_planes (contract in include/bdpt.h "Denoised planes") ----
int bdpt_bmfr_planes_prepare(bdpt_ctx* c, uint32_t numPlanes) {
  if (!c) return BDPT_E_INVALID;
  if (!c->haveSize) {
    fail(c, "bmfr_planes_prepare: bdpt_resize must be called first");
    return BDPT_E_STATE;
  }
  if (numPlanes < 1 || numPlanes > BDPT_BMFR_MAX_PLANES) {
    fail(c, "bmfr_planes_prepare: numPlanes must be 1 .. BDPT_BMFR_MAX_PLANES");
    return BDPT_E_INVALID;
  }
  ENTER(c);
  if (c->bmfrPlanes.accept && c->bmfrPlanes.slots >= numPlanes) return resetBmfrHistory(c, c->bmfrPlanes);
  return ensureBmfrHistory(c, c->bmfrPlanes, numPlanes, nullptr, "bmfr planes", kBmfrPlanesPrepare);
}

int bdpt_bmfr_planes_reset(bdpt_ctx* c) {
  if (!c) return BDPT_E_INVALID;
  return resetBmfrHistory(c, c->bmfrPlanes);
}

int bdpt_bmfr_execute_planes(bdpt_ctx* c, const bdpt_bmfr_params* p, const bdpt_gbuffer* g, const bdpt_bmfr_planes_desc* d, void* stream) {
  if (!c || !p || !g || !d) return BDPT_E_INVALID;
  if (int rc = bmfrCheck(c, g, "bmfr planes")) return rc;
  if (d->numPlanes < 1 || d->numPlanes > BDPT_BMFR_MAX_PLANES || d->reserved != 0 || !d->planes) {
    fail(c, "bmfr planes: numPlanes must be 1 .. BDPT_BMFR_MAX_PLANES, reserved 0 and planes set");
    return BDPT_E_INVALID;
  }
  if (d->prevPosition && !aligned(d->prevPosition, 16)) {
    fail(c, "bmfr planes: prevPosition not 16-byte aligned");
    return BDPT_E_INVALID;
  }
  const size_t n = (size_t)c->W * c->H;
  for (uint32_t k = 0; k < d->numPlanes; k++) {
    if (!aligned(d->planes[k], 16)) {
      fail(c, "bmfr planes: plane " + std::to_string(k) + " missing or not 16-byte aligned");
      return BDPT_E_INVALID;
    }
    for (uint32_t j = 0; j < k; j++) {
      const uintptr_t a = reinterpret_cast<uintptr_t>(d->planes[k]), b = reinterpret_cast<uintptr_t>(d->planes[j]);
      if (a < b + n * sizeof(float4) && b < a + n * sizeof(float4)) {
        fail(c, "bmfr planes: planes " + std::to_string(j) + " and " + std::to_string(k) + " overlap");
        return BDPT_E_INVALID;
      }
    }
  }
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = ensureBmfrHistory(c, c->bmfrPlanes, d->numPlanes, st, "bmfr planes", kBmfrPlanesPrepare)) return rc;
  return bmfrRun(c, c->bmfrPlanes, p, g, d->prevPosition, d->planes, d->numPlanes, st);
}

int bdpt_tile_pack(bdpt_ctx* c, const void* frame, void* packed, uint32_t bytesPerPixel, void* stream) {
  if (!c || !frame || !packed || (bytesPerPixel != 4 && bytesPerPixel != 8 && bytesPerPixel != 16)) return BDPT_E_INVALID;
  if (!c->haveSize) return BDPT_E_STATE;
  ENTER(c);
  launchTilePack(frame, packed, bytesPerPixel, c->P.pix, c->P.Np, reinterpret_cast<hipStream_t>(stream));
  HIPCHK(c, hipGetLastError());
  return BDPT_OK;
}
int bdpt_tile_unpack(bdpt_ctx* c, uint32_t owner, const void* packed, void* frame, uint32_t bytesPerPixel, void* stream) {
  if (!c || !frame || !packed || (bytesPerPixel != 4 && bytesPerPixel != 8 && bytesPerPixel != 16)) return BDPT_E_INVALID;
  if (!c->haveSize) return BDPT_E_STATE;
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (c->stripes.stripeRows == 0) {  // a band: its rows are one run
    if (owner != 0) return BDPT_E_INVALID;
    if (c->tileRows)
      HIPCHK(c, hipMemcpyAsync(static_cast<uint8_t*>(frame) + (size_t)c->rowRanges.front().first * c->W * bytesPerPixel, packed,
                               (size_t)c->tileRows * c->W * bytesPerPixel, hipMemcpyDeviceToDevice, st));
    return BDPT_OK;
  }
  if (owner >= c->stripes.numOwners) return BDPT_E_INVALID;
  launchTileUnpack(packed, frame, bytesPerPixel, c->W, c->H, c->stripes.stripeRows, c->stripes.numOwners, owner, c->sl.chunkRows, st);
  HIPCHK(c, hipGetLastError());
  return BDPT_OK;
}

int bdpt_splat_buffer(bdpt_ctx* c, uint64_t** out_ptr, uint64_t* out_n) {
  if (!c || !out_ptr) return BDPT_E_INVALID;
  if (!c->haveSize) return BDPT_E_STATE;
  *out_ptr = reinterpret_cast<uint64_t*>(c->splat);
  if (out_n) *out_n = (uint64_t)c->sl.owners * c->sl.chunkRows * c->W * 4;
  return BDPT_OK;
}

int bdpt_set_splat_buffer(bdpt_ctx* c, uint64_t* device_ptr, uint64_t num_u64) {
  if (!c) return BDPT_E_INVALID;
  if (!c->haveSize) return BDPT_E_STATE;
  if (!device_ptr) {
    c->splat = c->ownSplat;
    return BDPT_OK;
  }
  if (num_u64 < (uint64_t)c->sl.owners * c->sl.chunkRows * c->W * 4) {
    fail(c, "set_splat_buffer: buffer smaller than bdpt_get_tile_info's splatU64");
    return BDPT_E_INVALID;
  }
  c->splat = reinterpret_cast<unsigned long long*>(device_ptr);
  return BDPT_OK;
}

int bdpt_resolve(bdpt_ctx* c, const uint64_t* splat, uint32_t splat_row0, float* out, void* stream) {
  if (!c || !splat || !out) return BDPT_E_INVALID;
  if (!c->haveSize) return BDPT_E_STATE;
  const uint32_t firstRow = c->rowRanges.empty() ? 0 : c->rowRanges.front().first;
  if (splat_row0 > firstRow || (splat_row0 != 0 && c->sl.owners != 1)) {
    fail(c, "resolve: splat buffer does not cover the tile");
    return BDPT_E_INVALID;
  }
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  launchResolve(reinterpret_cast<const unsigned long long*>(splat), false, splat_row0, c->sl, out, c->W, c->P.pix, c->P.Np, st);
  HIPCHK(c, hipGetLastError());
  return BDPT_OK;
}

int bdpt_resolve_tile(bdpt_ctx* c, const uint64_t* tile_splat, float* out, void* stream) {
  if (!c || !tile_splat || !out) return BDPT_E_INVALID;
  if (!c->haveSize) return BDPT_E_STATE;
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  launchResolve(reinterpret_cast<const unsigned long long*>(tile_splat), true, 0, c->sl, out, c->W, c->P.pix, c->P.Np, st);
  HIPCHK(c, hipGetLastError());
  return BDPT_OK;
}

int bdpt_accumulate(bdpt_ctx* c, float* lastFrame, float* curFrame, uint32_t accumCount, uint32_t maxAccumCount,
                    uint64_t numTexels, void* stream) {
  if (!c || !lastFrame || !curFrame) return BDPT_E_INVALID;
  ENTER(c);
  launchAccumulate(lastFrame, curFrame, accumCount, maxAccumCount, numTexels, reinterpret_cast<hipStream_t>(stream));
  HIPCHK(c, hipGetLastError());
  return BDPT_OK;
}

int bdpt_accumulate_tile(bdpt_ctx* c, float* lastFrame, float* curFrame, uint32_t accumCount, uint32_t maxAccumCount, void* stream) {
  if (!c || !lastFrame || !curFrame) return BDPT_E_INVALID;
  if (!c->haveSize) return BDPT_E_STATE;
  ENTER(c);
  launchAccumulateTile(lastFrame, curFrame, accumCount, maxAccumCount, c->P.pix, c->P.Np, reinterpret_cast<hipStream_t>(stream));
  HIPCHK(c, hipGetLastError());
  return BDPT_OK;
}

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

int bdpt_get_counters(bdpt_ctx* c, bdpt_counters* out) {
  if (!c || !out) return BDPT_E_INVALID;
  if (!c->haveSize) return BDPT_E_STATE;
  ENTER(c);
  HIPCHK(c, hipStreamSynchronize(c->lastStream));
  DevCounters h;
  HIPCHK(c, hipMemcpy(&h, c->counters, sizeof(h), hipMemcpyDeviceToHost));
  static_assert(sizeof(bdpt_counters) == 17 * sizeof(uint64_t), "counter fields");
  uint64_t* o = reinterpret_cast<uint64_t*>(out);
  for (int f = 0; f < 13; f++) {
    o[f] = 0;
    for (uint32_t sh = 0; sh < kCounterShards; sh++) o[f] += h.v[sh][f];
  }
  out->alphaTestsClosest = out->alphaTestsShadow = out->hintedNee = out->hintedSplat = 0;
  for (uint32_t sh = 0; sh < kCounterShards; sh++) {
    out->alphaTestsClosest += h.v[sh][C_ALPHA_CLOSEST];
    out->alphaTestsShadow += h.v[sh][C_ALPHA_SHADOW];
    out->hintedNee += h.v[sh][C_HINT_NEE];
    out->hintedSplat += h.v[sh][C_HINT_SPLAT];
  }
  out->raysPrimary = (uint64_t)c->P.Np;  // GBufferRayGen traces exactly one ray per tile pixel
  return BDPT_OK;
}

int bdpt_enable_stage_timing(bdpt_ctx* c, int enable) {
  if (!c) return BDPT_E_INVALID;
  c->timing = enable != 0;
  return BDPT_OK;
}

int bdpt_get_stage_times(bdpt_ctx* c, const char** names, float* ms, int cap) {
  if (!c || !names || !ms) return BDPT_E_INVALID;
  if (!c->timing || c->numStages == 0) return 0;
  ENTER(c);
  HIPCHK(c, hipEventSynchronize(c->ev[c->numStages]));
  int n = std::min(cap, c->numStages);
  for (int i = 0; i < n; i++) {
    names[i] = c->stageNames[i];
    float t = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&t, c->ev[i], c->ev[i + 1]));
    ms[i] = t;
  }
  // the second stream's kernels, behind the caller's stages ("side:" names; the caller's stream joined them before its end)
  for (int i = 0; i < c->numSideStages && n < cap; i++, n++) {
    names[n] = c->sideNames[i];
    float t = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&t, c->sideEv[2 * i], c->sideEv[2 * i + 1]));
    ms[n] = t;
  }
  return n;
}

int bdpt_sync(bdpt_ctx* c, void* stream) {
  if (!c) return BDPT_E_INVALID;
  ENTER(c);
  HIPCHK(c, hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
  return BDPT_OK;
}

// ---- test hooks --------------------------------------------------------------------------------
int bdpt_test_rng(bdpt_ctx* c, const uint32_t* val0, const uint32_t* val1, uint32_t n, uint32_t draws, uint32_t* out_states,
                  float* out_floats) {
  if (!c || !val0 || !val1 || !out_states || !out_floats) return BDPT_E_INVALID;
  ENTER(c);
  std::vector<void*> pool;
  const uint32_t *d0, *d1;
  uint32_t* ds;
  float* df;
  int rc;
  if ((rc = devUpload(c, pool, &d0, val0, n)) || (rc = devUpload(c, pool, &d1, val1, n)) ||
      (rc = devAlloc(c, pool, &ds, (size_t)n * draws)) || (rc = devAlloc(c, pool, &df, (size_t)n * draws))) {
    freePool(pool);
    return rc;
  }
  launchTestRng(d0, d1, n, draws, ds, df, nullptr);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out_states, ds, (size_t)n * draws * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out_floats, df, (size_t)n * draws * 4, hipMemcpyDeviceToHost);
  freePool(pool);
  if (e != hipSuccess) {
    fail(c, hipGetErrorString(e));
    return BDPT_E_HIP;
  }
  return BDPT_OK;
}

int bdpt_test_trace(bdpt_ctx* c, const float* rays, uint32_t n, int mode, int32_t* out_prim, float* out_tuv) {
  if (!c || !rays || !out_prim || !out_tuv || mode < 0 || mode > 2) return BDPT_E_INVALID;
  if (!c->haveScene) return BDPT_E_STATE;
  ENTER(c);
  std::vector<void*> pool;
  const float* dr;
  int32_t* dp;
  float* dt;
  int rc;
  if ((rc = devUpload(c, pool, &dr, rays, (size_t)n * 8)) || (rc = devAlloc(c, pool, &dp, n)) ||
      (rc = devAlloc(c, pool, &dt, (size_t)n * 3))) {
    freePool(pool);
    return rc;
  }
  launchTestTrace(c->S, dr, n, mode, dp, dt, nullptr);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out_prim, dp, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out_tuv, dt, (size_t)n * 12, hipMemcpyDeviceToHost);
  freePool(pool);
  if (e != hipSuccess) {
    fail(c, hipGetErrorString(e));
    return BDPT_E_HIP;
  }
  return BDPT_OK;
}

int bdpt_test_trace_shadow(bdpt_ctx* c, const float* rays, uint32_t n, uint8_t* out_vis, uint32_t* out_max_stack) {
  if (!c || !rays || !out_vis || !n) return BDPT_E_INVALID;
  if (!c->haveScene) return BDPT_E_STATE;
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
  std::vector<void*> pool;
  const float* dp;
  const uint32_t* dc;
  uint8_t* dv;
  DevCounters* dcnt;
  int rc;
  if ((rc = devUpload(c, pool, &dp, planes.data(), planes.size())) || (rc = devUpload(c, pool, &dc, cursors.data(), cursors.size())) ||
      (rc = devAlloc(c, pool, &dv, (size_t)n)) || (rc = devAlloc(c, pool, &dcnt, 1))) {
    freePool(pool);
    return rc;
  }
  hipError_t e = hipMemset(dcnt, 0, sizeof(DevCounters));
  if (e == hipSuccess) {
    launchTestTraceShadow(c->S, dp, n, dc, const_cast<uint32_t*>(dc) + kCursorStride, dv, dcnt, rays[6], c->numCUs, nullptr);
    e = hipDeviceSynchronize();
  }
  DevCounters h;
  if (e == hipSuccess) e = hipMemcpy(out_vis, dv, (size_t)n, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(&h, dcnt, sizeof(h), hipMemcpyDeviceToHost);
  freePool(pool);
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

int bdpt_get_area_light_info(bdpt_ctx* c, bdpt_area_light_info* out) {
  if (!c || !out) return BDPT_E_INVALID;
  if (!c->haveScene) {
    fail(c, "area_light_info: no scene (bdpt_set_scene first)");
    return BDPT_E_STATE;
  }
  ENTER(c);
  if (int rc = ensureAreaLights(c, nullptr)) return rc;
  HIPCHK(c, hipDeviceSynchronize());  // (the last update's refresh)
  *out = bdpt_area_light_info{};
  out->numEmitters = c->area.n;
  out->numTextured = c->areaTextured;
  if (c->area.n) HIPCHK(c, hipMemcpy(&out->totalWeight, c->area.total, sizeof(float), hipMemcpyDeviceToHost));
  return BDPT_OK;
}

int bdpt_test_area_light_sample(bdpt_ctx* c, uint32_t mode, const uint32_t* states, const float* points, uint32_t n, float* out) {
  if (!c || !states || !out || mode > 1 || (mode == 1 && !points)) return BDPT_E_INVALID;
  if (!c->haveScene) {
    fail(c, "test_area_light_sample: no scene");
    return BDPT_E_STATE;
  }
  ENTER(c);
  if (int rc = ensureAreaLights(c, nullptr)) return rc;
  if (!n) return BDPT_OK;
  std::vector<void*> pool;
  const uint32_t* ds = nullptr;
  const float* dp = nullptr;
  float* dout = nullptr;
  int rc;
  if ((rc = devUpload(c, pool, &ds, states, n)) || (mode == 1 && (rc = devUpload(c, pool, &dp, points, (size_t)n * 3))) ||
      (rc = devAlloc(c, pool, &dout, (size_t)n * 16))) {
    freePool(pool);
    return rc;
  }
  hipError_t e = hipDeviceSynchronize();  // (the last update's refresh)
  if (e == hipSuccess) {
    if (c->area.n)
      launchTestAreaSample(c->S, c->area, (int)mode, ds, dp, n, dout, nullptr);
    else
      e = hipMemset(dout, 0, (size_t)n * 64);  // no emitter: every output is zero
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)n * 64, hipMemcpyDeviceToHost);
  freePool(pool);
  if (e != hipSuccess) {
    fail(c, hipGetErrorString(e));
    return BDPT_E_HIP;
  }
  return BDPT_OK;
}

int bdpt_test_alpha(bdpt_ctx* c, uint32_t variant, const uint32_t* prim, const float* uv, uint32_t n, uint8_t* out_fails) {
  if (!c || !prim || !uv || !out_fails || variant > 2) return BDPT_E_INVALID;
  if (!c->haveScene) {
    fail(c, "test_alpha: no scene");
    return BDPT_E_STATE;
  }
  ENTER(c);
  for (uint32_t i = 0; i < n; i++)
    if (prim[i] >= c->numTriangles) {
      fail(c, "test_alpha: a prim is not a triangle of the scene");
      return BDPT_E_INVALID;
    }
  if (!n) return BDPT_OK;
  std::vector<void*> pool;
  const uint32_t* dp = nullptr;
  const float* duv = nullptr;
  uint8_t* dout = nullptr;
  int rc;
  if ((rc = devUpload(c, pool, &dp, prim, n)) || (rc = devUpload(c, pool, &duv, uv, (size_t)n * 2)) || (rc = devAlloc(c, pool, &dout, (size_t)n))) {
    freePool(pool);
    return rc;
  }
  launchTestAlpha(c->S, c->alphaTris, c->alphaTris ? c->numAlphaTris : 0u, variant, dp, duv, n, dout, nullptr);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out_fails, dout, (size_t)n, hipMemcpyDeviceToHost);
  freePool(pool);
  if (e != hipSuccess) {
    fail(c, hipGetErrorString(e));
    return BDPT_E_HIP;
  }
  return BDPT_OK;
}

int bdpt_test_bsdf(bdpt_ctx* c, const float* in, uint32_t n, uint32_t matIndex, float* out) {
  if (!c || !in || !out) return BDPT_E_INVALID;
  ENTER(c);
  std::vector<void*> pool;
  const float* di;
  float* dout;
  int rc;
  if ((rc = devUpload(c, pool, &di, in, (size_t)n * 20)) || (rc = devAlloc(c, pool, &dout, (size_t)n * 16))) {
    freePool(pool);
    return rc;
  }
  launchTestBsdf(di, n, matIndex, dout, nullptr);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)n * 64, hipMemcpyDeviceToHost);
  freePool(pool);
  if (e != hipSuccess) {
    fail(c, hipGetErrorString(e));
    return BDPT_E_HIP;
  }
  return BDPT_OK;
}

}  // extern "C"
