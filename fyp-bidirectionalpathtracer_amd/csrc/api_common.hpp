// api_common.hpp — what the files that implement entry points (api*.cpp) share: error reporting, the device switch, the
// refusals every call spells alike, device allocation into a pool, and the few functions one topic needs of another.
// Internal to the library.
#pragma once
#include <algorithm>
#include <string>

#include "context.hpp"
#include "launch.hpp"

namespace bdpt {

inline bool fail(bdpt_ctx* c, const std::string& m) {
  if (c) c->err = m;
  return false;
}
#define HIPCHK(ctx, expr)                                                                       \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess) {                                                                     \
      bdpt::fail(ctx, std::string(#expr) + ": " + hipGetErrorString(e_));                             \
      return BDPT_E_HIP;                                                                        \
    }                                                                                           \
  } while (0)

// Every entry point that launches or allocates starts here: the context's device becomes current, so one
// host thread can hold contexts on several GPUs.
#define ENTER(ctx) HIPCHK(ctx, hipSetDevice((ctx)->device))

// a pointer that is set and a multiple of `a` bytes
inline bool aligned(const void* p, uintptr_t a) { return p && (reinterpret_cast<uintptr_t>(p) % a) == 0; }

// "<what>: <why>" as the context's error; returns `code`
inline int refuse(bdpt_ctx* c, int code, const char* what, const char* why) {
  fail(c, std::string(what) + ": " + why);
  return code;
}
inline int needScene(bdpt_ctx* c, const char* what) {
  return c->scene.have ? BDPT_OK : refuse(c, BDPT_E_STATE, what, "no scene (bdpt_set_scene first)");
}
inline int needCamera(bdpt_ctx* c, const char* what) {
  return c->haveCamera ? BDPT_OK : refuse(c, BDPT_E_STATE, what, "no camera (bdpt_set_camera first)");
}

inline bool streamIsCapturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) return false;
  return cs != hipStreamCaptureStatusNone;
}

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

template <class T>
int devAlloc(bdpt_ctx* c, DevPool& pool, T** out, size_t count) {
  void* p = nullptr;
  size_t bytes = std::max<size_t>(count * sizeof(T), 16);
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) {
    fail(c, std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
    return BDPT_E_NOMEM;
  }
  pool.ptrs.push_back(p);
  *out = reinterpret_cast<T*>(p);
  return BDPT_OK;
}
template <class T>
int devUpload(bdpt_ctx* c, DevPool& pool, const T** out, const T* host, size_t count) {
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

// api.cpp — the drops; the device is idle, or the caller has synchronised it
void dropMorph(MorphState& m);
void dropSkin(SkinState& k);  // and its morph
void dropLightGroups(LightGroups& g);
void dropBmfrHistory(BmfrHistory& h);
void dropEnv(EnvState& e);
void dropScene(bdpt_ctx* c);  // and its skin, its morph, the light groups
void dropFrame(bdpt_ctx* c);  // and both histories, the light groups
// the call is ordered after everything this context enqueued before (its last stream joins its side stream)
int orderAfterLast(bdpt_ctx* c, hipStream_t st);

// api_scene.cpp — the emitter table of area lights (area_lights.hip); synchronises, so not while capturing
int ensureAreaLights(bdpt_ctx* c, hipStream_t st);
// api_deform.cpp — the refit plan and its scratch, the regions of the tree as built, the previous pose; not while capturing
int ensureRefit(bdpt_ctx* c, hipStream_t st);
int ensureRefitPieces(bdpt_ctx* c);
int allocPrevPose(bdpt_ctx* c);
// api_bmfr.cpp — history for at least `slots` images; the single-image history's arguments are (c, c->frame.bmfr, 1, st,
// "bmfr", kBmfrPrepare)
constexpr const char* kBmfrPrepare = "bdpt_prepare(BDPT_PREPARE_BMFR)";
int ensureBmfrHistory(bdpt_ctx* c, BmfrHistory& h, uint32_t slots, hipStream_t st, const char* who, const char* prepare);

}  // namespace bdpt
