// api_bmfr.cpp — the denoiser of the C ABI (include/bdpt.h): the history (context.hpp BmfrHistory) and the bdpt_bmfr_*
// calls.  bdpt_bmfr_execute, _execute_motion and _execute_planes neither allocate nor synchronise once their history
// exists (bdpt_prepare(BDPT_PREPARE_BMFR), bdpt_bmfr_planes_prepare), so they can be captured; without it the first call
// allocates it, and refuses (BDPT_E_STATE) while the stream is being captured.  The reset, save and load calls synchronise.
#include <string>

#include "api_common.hpp"

using namespace bdpt;

namespace {
// (kBmfrPrepare, api_common.hpp, and this: the calls that allocate a history ahead of a stream capture, as the refusal
// inside a capture names them)
constexpr const char* kBmfrPlanesPrepare = "bdpt_bmfr_planes_prepare";

int resetBmfrHistory(bdpt_ctx* c, BmfrHistory& h) {
  if (!h.accept) return BDPT_OK;  // nothing allocated yet
  ENTER(c);
  const size_t n = (size_t)c->frame.W * c->frame.H;
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
}  // namespace

// (declared in api_common.hpp)  (Re)allocating resets; replacing a smaller history waits for the device first
// (frames in flight still use it), the first allocation frees nothing and does not wait.  Not while `st` is being
// captured: the message names `who` and the call (`prepare`) that allocates ahead of the capture.
int bdpt::ensureBmfrHistory(bdpt_ctx* c, BmfrHistory& h, uint32_t slots, hipStream_t st, const char* who, const char* prepare) {
  if (h.accept && h.slots >= slots) return BDPT_OK;
  if (streamIsCapturing(st)) {
    fail(c, std::string(who) + ": the history needs " + prepare + " before stream capture");
    return BDPT_E_STATE;
  }
  if (h.accept) {
    HIPCHK(c, hipDeviceSynchronize());
    dropBmfrHistory(h);
  }
  const size_t n = std::max<size_t>((size_t)c->frame.W * c->frame.H, 1);
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

extern "C" {

// BlockwiseMultiOrderFeatureRegression::execute (DenoisePass.cpp:146-204)
namespace {
// what every denoise entry point checks first
int bmfrCheck(bdpt_ctx* c, const bdpt_gbuffer* g, const char* who) {
  if (!c->frame.have) {
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
  const size_t n = (size_t)c->frame.W * c->frame.H;
  BmfrDev A{};
  A.W = c->frame.W;
  A.H = c->frame.H;
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
  if (int rc = ensureBmfrHistory(c, c->frame.bmfr, 1, st, "bmfr", kBmfrPrepare)) return rc;
  return bmfrRun(c, c->frame.bmfr, p, g, prevPosition, &noisy, 1, st);
}
}  // namespace

int bdpt_bmfr_execute(bdpt_ctx* c, const bdpt_bmfr_params* p, const bdpt_gbuffer* g, float* noisy, void* stream) {
  if (!c || !p || !g || !noisy) return BDPT_E_INVALID;
  return bmfrSingle(c, p, g, nullptr, noisy, stream);
}

int bdpt_bmfr_execute_motion(bdpt_ctx* c, const bdpt_bmfr_params* p, const bdpt_gbuffer* g, const float* prevPosition, float* noisy,
                             void* stream) {
  if (!c || !p || !g || !noisy) return BDPT_E_INVALID;
  if (!aligned(prevPosition, 16)) return refuse(c, BDPT_E_INVALID, "bmfr_execute_motion", "prevPosition missing or not 16-byte aligned");
  return bmfrSingle(c, p, g, prevPosition, noisy, stream);
}

int bdpt_bmfr_reset(bdpt_ctx* c) {
  if (!c) return BDPT_E_INVALID;
  return resetBmfrHistory(c, c->frame.bmfr);
}

// [pos | norm | noisy | filtered] of the read side (slot 0 of the single-image history), W * H float4 each
int bdpt_bmfr_history_bytes(const bdpt_ctx* c, uint64_t* out_bytes) {
  if (!c || !out_bytes) return BDPT_E_INVALID;
  *out_bytes = (c->frame.have && c->frame.bmfr.accept) ? (uint64_t)c->frame.W * c->frame.H * sizeof(float4) * 4 : 0;
  return BDPT_OK;
}
int bdpt_bmfr_save_history(bdpt_ctx* c, void* blob, uint64_t bytes) {
  if (!c || !blob) return BDPT_E_INVALID;
  if (!c->frame.have || !c->frame.bmfr.accept) {
    fail(c, "bmfr_save_history: no history (the denoiser has not run on this context)");
    return BDPT_E_STATE;
  }
  const size_t n = (size_t)c->frame.W * c->frame.H, plane = n * sizeof(float4);
  if (bytes < 4 * plane) return BDPT_E_INVALID;
  ENTER(c);
  HIPCHK(c, hipStreamSynchronize(c->lastStream));
  const BmfrHistory& h = c->frame.bmfr;
  const float4* src[4] = {h.pos[h.read], h.norm[h.read], h.noisy + h.read * n, h.filtered + h.read * n};
  for (int k = 0; k < 4; k++) HIPCHK(c, hipMemcpy(static_cast<uint8_t*>(blob) + k * plane, src[k], plane, hipMemcpyDeviceToHost));
  return BDPT_OK;
}
int bdpt_bmfr_load_history(bdpt_ctx* c, const void* blob, uint64_t bytes) {
  if (!c || !blob) return BDPT_E_INVALID;
  if (!c->frame.have) return refuse(c, BDPT_E_STATE, "bmfr_load_history", "bdpt_resize must be called first");
  const size_t n = (size_t)c->frame.W * c->frame.H, plane = n * sizeof(float4);
  if (bytes != 4 * plane) return refuse(c, BDPT_E_INVALID, "bmfr_load_history", "the blob was written for another frame size");
  ENTER(c);
  if (int rc = ensureBmfrHistory(c, c->frame.bmfr, 1, nullptr, "bmfr", kBmfrPrepare)) return rc;  // (a new one is reset: read side 0)
  HIPCHK(c, hipStreamSynchronize(c->lastStream));
  const BmfrHistory& h = c->frame.bmfr;
  float4* dst[4] = {h.pos[h.read], h.norm[h.read], h.noisy + h.read * n, h.filtered + h.read * n};
  for (int k = 0; k < 4; k++) HIPCHK(c, hipMemcpy(dst[k], static_cast<const uint8_t*>(blob) + k * plane, plane, hipMemcpyHostToDevice));
  return BDPT_OK;
}

// ---- bdpt_bmfr_execute_planes (contract in include/bdpt.h "Denoised planes") ----
int bdpt_bmfr_planes_prepare(bdpt_ctx* c, uint32_t numPlanes) {
  if (!c) return BDPT_E_INVALID;
  if (!c->frame.have) return refuse(c, BDPT_E_STATE, "bmfr_planes_prepare", "bdpt_resize must be called first");
  if (numPlanes < 1 || numPlanes > BDPT_BMFR_MAX_PLANES) {
    fail(c, "bmfr_planes_prepare: numPlanes must be 1 .. BDPT_BMFR_MAX_PLANES");
    return BDPT_E_INVALID;
  }
  ENTER(c);
  if (c->frame.bmfrPlanes.accept && c->frame.bmfrPlanes.slots >= numPlanes) return resetBmfrHistory(c, c->frame.bmfrPlanes);
  return ensureBmfrHistory(c, c->frame.bmfrPlanes, numPlanes, nullptr, "bmfr planes", kBmfrPlanesPrepare);
}

int bdpt_bmfr_planes_reset(bdpt_ctx* c) {
  if (!c) return BDPT_E_INVALID;
  return resetBmfrHistory(c, c->frame.bmfrPlanes);
}

int bdpt_bmfr_execute_planes(bdpt_ctx* c, const bdpt_bmfr_params* p, const bdpt_gbuffer* g, const bdpt_bmfr_planes_desc* d, void* stream) {
  if (!c || !p || !g || !d) return BDPT_E_INVALID;
  if (int rc = bmfrCheck(c, g, "bmfr planes")) return rc;
  if (d->numPlanes < 1 || d->numPlanes > BDPT_BMFR_MAX_PLANES || d->reserved != 0 || !d->planes) {
    fail(c, "bmfr planes: numPlanes must be 1 .. BDPT_BMFR_MAX_PLANES, reserved 0 and planes set");
    return BDPT_E_INVALID;
  }
  if (d->prevPosition && !aligned(d->prevPosition, 16)) return refuse(c, BDPT_E_INVALID, "bmfr planes", "prevPosition not 16-byte aligned");
  const size_t n = (size_t)c->frame.W * c->frame.H;
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
  if (int rc = ensureBmfrHistory(c, c->frame.bmfrPlanes, d->numPlanes, st, "bmfr planes", kBmfrPlanesPrepare)) return rc;
  return bmfrRun(c, c->frame.bmfrPlanes, p, g, d->prevPosition, d->planes, d->numPlanes, st);
}

}  // extern "C"
