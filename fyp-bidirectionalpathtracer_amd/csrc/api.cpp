// api.cpp — the context itself: bdpt_create / bdpt_destroy, the drops that end each lifetime of context.hpp, the ordering
// of a call after the context's last one, and the read-backs (last error, counters, stage times, bdpt_sync).  The rest
// of the C ABI of include/bdpt.h is split by topic: api_scene.cpp, api_deform.cpp, api_frame.cpp, api_bmfr.cpp,
// api_query.cpp, api_test.cpp.  bdpt_create and bdpt_destroy allocate and synchronise; bdpt_get_counters,
// bdpt_get_stage_times and bdpt_sync wait for a stream; none may be captured.  Every entry point that launches or
// allocates makes the context's device current first, so one host thread may drive contexts on several GPUs;
// per-context launch state (persistent grid sizes, counters read-back) lives in bdpt_ctx, never in statics.
#include "api_common.hpp"

using namespace bdpt;

// ---- the drops (declared in api_common.hpp): free what the struct owns, then reset it to its member initialisers.
// Assigning a fresh value does both for what a DevPool holds, members below it included: a skin takes its morph along
// (the morph's base and outputs were that skin's), a scene its skin. ----
void bdpt::dropMorph(MorphState& m) { m = MorphState{}; }
void bdpt::dropSkin(SkinState& k) { k = SkinState{}; }
void bdpt::dropLightGroups(LightGroups& g) {
  if (g.splat) (void)hipFree(g.splat);
  if (g.lightIdx) (void)hipFree(g.lightIdx);
  g = LightGroups{};
}
void bdpt::dropBmfrHistory(BmfrHistory& h) {
  for (void* p : {(void*)h.pos[0], (void*)h.pos[1], (void*)h.norm[0], (void*)h.norm[1], (void*)h.noisy, (void*)h.filtered, (void*)h.accept,
                  (void*)h.prevPixel})
    if (p) (void)hipFree(p);
  h = BmfrHistory{};
}
void bdpt::dropEnv(EnvState& e) { e = EnvState{}; }
void bdpt::dropScene(bdpt_ctx* c) {
  dropLightGroups(c->groups);
  c->scene = SceneState{};
  c->scene.S.stackOvf = c->stackOvf;  // the one place the context's members of SceneDev are set
  c->scene.S.stackOvfStride = c->stackOvfStride;
}
void bdpt::dropFrame(bdpt_ctx* c) {
  dropLightGroups(c->groups);
  dropBmfrHistory(c->frame.bmfr);
  dropBmfrHistory(c->frame.bmfrPlanes);
  c->frame = FrameState{};
}

int bdpt::orderAfterLast(bdpt_ctx* c, hipStream_t st) {
  if (c->lastStream != st) {
    HIPCHK(c, hipEventRecord(c->evOrder, c->lastStream));
    HIPCHK(c, hipStreamWaitEvent(st, c->evOrder, 0));
  }
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
  dropFrame(c);
  dropScene(c);
  dropEnv(c->envTable);
  if (c->stackOvf) (void)hipFree(c->stackOvf);
  if (c->rayCursor) (void)hipFree(c->rayCursor);
  if (c->adaptiveSum) (void)hipFree(c->adaptiveSum);
  if (c->evCreated) {
    for (int i = 0; i <= kMaxStages; i++) (void)hipEventDestroy(c->ev[i]);
    for (hipEvent_t e : c->sideEv) (void)hipEventDestroy(e);
  }
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

int bdpt_get_counters(bdpt_ctx* c, bdpt_counters* out) {
  if (!c || !out) return BDPT_E_INVALID;
  if (!c->frame.have) return BDPT_E_STATE;
  ENTER(c);
  HIPCHK(c, hipStreamSynchronize(c->lastStream));
  DevCounters h;
  HIPCHK(c, hipMemcpy(&h, c->frame.counters, sizeof(h), hipMemcpyDeviceToHost));
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
  out->raysPrimary = (uint64_t)c->frame.P.Np;  // GBufferRayGen traces exactly one ray per tile pixel
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

}  // extern "C"
