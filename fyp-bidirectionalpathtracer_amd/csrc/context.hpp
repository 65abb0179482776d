// context.hpp — the context behind the C ABI (include/bdpt.h) and what every file that implements entry points needs:
// error reporting, the device switch, the ordering of a call after the context's last one.  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

#include "../../include/bdpt.h"
#include "bvh.h"
#include "kernels.h"
#include "morph.h"
#include "refit.h"
#include "skin.h"

namespace bdpt {
constexpr int kMaxStages = 64;

// What the denoiser keeps between frames for `slots` images over one G-buffer: position / normal ping-pong pairs, accept
// and prevPixel once, noisy and filtered pairs per slot (side s of slot k at [(2 * k + s) * W * H]).  Own allocations, not
// frameAllocs: growing frees them; bdpt_resize and bdpt_destroy drop them (the history goes with the frame,
// BlockwiseMultiOrderFeatureRegression::resize).
struct BmfrHistory {
  float4* pos[2] = {nullptr, nullptr};
  float4* norm[2] = {nullptr, nullptr};
  float4 *noisy = nullptr, *filtered = nullptr;
  uint8_t* accept = nullptr;  // set: the history is allocated
  uint32_t* prevPixel = nullptr;
  uint32_t slots = 0;
  int read = 0;  // which side holds the previous frame
};
}  // namespace bdpt

struct bdpt_ctx {
  int device = 0;
  int numCUs = 256;
  std::string err;
  // scene
  bool haveScene = false, haveCamera = false, haveSize = false;
  bdpt::SceneDev S{};
  std::vector<void*> sceneAllocs;
  bdpt_bvh_info bvhInfo{};
  bdpt_camera cam{};
  bdpt_environment env{};  // bdpt_set_environment: what BDPT_PARAM_ENV_ON_MISS looks up (none: black)
  // frame
  uint32_t W = 0, H = 0, maxDepth = 0;
  // the tile: which frame rows this context renders (a contiguous band, or the stripes of one owner) and where
  // splat accumulators live (SplatLayout); rows in ascending order
  std::vector<std::pair<uint32_t, uint32_t>> rowRanges;  // [first, last) runs of rows
  uint32_t tileRows = 0;
  bdpt::SplatLayout sl{1, 1, 0};
  bdpt_stripes stripes{0, 1, 0};  // stripeRows == 0: contiguous band (bdpt_resize)
  bdpt::PathBuf P{};
  std::vector<void*> frameAllocs;
  unsigned long long* splat = nullptr;     // buffer in use (own or caller-provided)
  unsigned long long* ownSplat = nullptr;
  bdpt::DevCounters* counters = nullptr;
  hipStream_t lastStream = nullptr;
  // stage timing
  bool timing = false;
  hipEvent_t ev[bdpt::kMaxStages + 1]{};
  const char* stageNames[bdpt::kMaxStages]{};
  int numStages = 0;
  bool evCreated = false;
  // kernels on the context's second stream (the splat and connection generators): their own event pairs, so that a
  // kernel's time is the kernel's and the caller's stream shows the WAIT for it as a stage of its own
  static constexpr int kMaxSideStages = 4;
  hipEvent_t sideEv[2 * kMaxSideStages]{};
  const char* sideNames[kMaxSideStages]{};
  int numSideStages = 0;
  int lazyRounds = 3;
  bdpt::LaunchGrids grids{};  // persistent-grid sizes for this context's device
  int* stackOvf = nullptr;      // overflow rows of the persistent kernels' traversal stacks (kernels.h kStackLds)
  uint32_t stackOvfStride = 0;  // lanes per row: every wave a persistent grid can hold
  unsigned long long* rayCursor = nullptr;  // fetch cursor and done count of bdpt_trace_rays (each launch leaves them zero)
  unsigned long long* adaptiveSum = nullptr;  // active-pixel sum and done count of bdpt_adaptive_update (each launch leaves them zero)
  // channels of the built-in primary stage (bdpt_execute with in == NULL): bdpt_prepare or first use
  bdpt_gbuffer ownGb{};
  // BMFR history, two of them and apart: bmfr for bdpt_bmfr_execute / _motion (one slot; bdpt_prepare(BDPT_PREPARE_BMFR)
  // or the first call), bmfrPlanes for bdpt_bmfr_execute_planes (bdpt_bmfr_planes_prepare or the first call that needs
  // more slots)
  bdpt::BmfrHistory bmfr, bmfrPlanes;
  // the splat and NEE generators run beside the connection generator on this stream (fork/join with events; capture-safe)
  hipStream_t walkStream = nullptr;
  hipEvent_t evFork = nullptr, evJoin = nullptr, evSplat = nullptr;
  // occluder hints (kernels.hip "Occluder hints"): the primary-visibility triangle of every frame pixel, written by this
  // context's G-buffer pass and read by its light-tracing generator.  BDPT_NO_HINTS (environment) switches both kinds off.
  uint32_t* hintPix = nullptr;
  bool hints = true;
  // a context that renders only part of the frame fills the hints of ALL frame pixels when its camera changes (its
  // light-tracing rays aim anywhere); its own rows are refreshed by every G-buffer pass
  bdpt_camera hintCam{};
  bool hintCamValid = false;
  // refit (bdpt_update_geometry / bdpt_set_lights): the plan and its scratch are made on first use or by
  // bdpt_prepare(BDPT_PREPARE_REFIT) and live in sceneAllocs (a new scene drops them)
  uint32_t numVertices = 0, numTriangles = 0;
  uint32_t* lightMaps = nullptr;  // = S.lightMap (writable)
  bool refitReady = false;
  bdpt::BvhRefitPlan refitPlan;  // (host copy: the SAH of bdpt_get_refit_info walks it)
  bdpt::RefitDev refit{};
  uint32_t numUpdates = 0;
  float* stage[3] = {nullptr, nullptr, nullptr};  // device copies of host-pointer inputs: positions, normals, bitangents
  // host-pointer inputs go through pinned memory (copied before the call returns); evStage marks the end of the copy
  // that last read it
  void* pinned = nullptr;
  size_t pinnedBytes = 0;
  hipEvent_t evStage = nullptr, evOrder = nullptr;
  bool stageInFlight = false;
  // light groups (bdpt_execute_light_groups, bdpt_execute_grouped): the splat-value planes (groupSplatPlanes of them) and
  // each pixel's light, made by bdpt_prepare(BDPT_PREPARE_LIGHT_GROUPS / _LIGHT_GROUP_TABLE) or by the first call that
  // needs more planes than there are; they depend on the scene's light count and the frame size, so bdpt_set_scene and
  // bdpt_resize drop them
  unsigned long long* groupSplat = nullptr;
  uint32_t groupSplatPlanes = 0;
  uint8_t* groupLightIdx = nullptr;
  // area lights (BDPT_PARAM_AREA_LIGHTS): the emitter table, made by bdpt_prepare(BDPT_PREPARE_AREA_LIGHTS) or the first
  // frame with the switch, in sceneAllocs (a new scene drops it); refreshed on the device by every bdpt_update_geometry.
  // alphaTris: the non-opaque triangles in ascending order (their alpha-test records' order), kept for the table build.
  const uint32_t* alphaTris = nullptr;
  uint32_t numAlphaTris = 0;
  bool areaReady = false;
  bdpt::AreaDev area{};
  uint32_t areaTextured = 0;
  float* areaBlockSum = nullptr;     // one float and one word per 64 emitters: the refresh's scratch
  uint32_t* areaBlockLast = nullptr;
  // skinning (bdpt_set_skin): the rest streams, weights, ids, the skinned streams and the device palettes, in skinAllocs
  // (bdpt_set_skin and bdpt_set_scene drop them).  skinPalette: where host-pointer palettes are staged (bones, normalBones).
  std::vector<void*> skinAllocs;
  bool haveSkin = false;
  bdpt::SkinDev skin{};
  float* skinPalette[2] = {nullptr, nullptr};
  // morph targets (bdpt_set_morph): the vertex-major entries, the active-vertex list, without a skin the base and the
  // morphed streams, and the device weights, in morphAllocs (bdpt_set_morph, bdpt_set_skin and bdpt_set_scene drop
  // them).  morphWeights: where host-pointer weights are staged.
  std::vector<void*> morphAllocs;
  bool haveMorph = false;
  bdpt::MorphDev morph{};
  float* morphWeights = nullptr;
  // motion (bdpt_prepare(BDPT_PREPARE_MOTION)): the previous pose, three float4 per primitive, in sceneAllocs (a new scene
  // drops it); bdpt_keep_pose copies the current corners into it
  float4* prevPose = nullptr;
};

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

// api.cpp
// the call is ordered after everything this context enqueued before (its last stream joins its side stream)
int orderAfterLast(bdpt_ctx* c, hipStream_t st);
// The emitter table of area lights (area_lights.hip); synchronises, so not while capturing.
int ensureAreaLights(bdpt_ctx* c, hipStream_t st);

}  // namespace bdpt
