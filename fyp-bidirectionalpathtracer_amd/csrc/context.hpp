// context.hpp — the context behind the C ABI (include/bdpt.h): its state, grouped by the call that drops it.
//   SceneState   what bdpt_set_scene replaces; below it SkinState (bdpt_set_skin), below that MorphState (bdpt_set_morph):
//                dropping a scene drops its skin, dropping a skin drops its morph
//   FrameState   what bdpt_resize / bdpt_resize_stripes replace
//   LightGroups  sized by the scene's lights and by the frame: both drops drop them
//   EnvState     what bdpt_set_environment replaces: the sampling table bdpt_env_prepare made for the map
//   bdpt_ctx     these, and what lives as long as the context (device, streams, events, cursors, staging, timing)
// Every default is a member initialiser, so a drop is "free what the struct owns, then x = X{}" (api.cpp dropScene,
// dropSkin, dropMorph, dropFrame, dropLightGroups: the only places that reset a field).  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

#include "../../include/bdpt.h"
#include "bvh.h"
#include "env_light.h"
#include "kernels.h"
#include "morph.h"
#include "refit.h"
#include "skin.h"

namespace bdpt {
constexpr int kMaxStages = 64;

// Device allocations with one owner: freed when the pool goes (or release()), handed over as a whole by moveTo.  The
// device they came from is idle, or the caller has synchronised it, by then.
struct DevPool {
  std::vector<void*> ptrs;
  DevPool() = default;
  DevPool(DevPool&& o) noexcept : ptrs(std::move(o.ptrs)) { o.ptrs.clear(); }
  DevPool& operator=(DevPool&& o) noexcept {
    if (this != &o) {
      release();
      ptrs = std::move(o.ptrs);
      o.ptrs.clear();
    }
    return *this;
  }
  ~DevPool() { release(); }
  void release() {
    for (void* p : ptrs) (void)hipFree(p);
    ptrs.clear();
  }
  // commit: `to` owns these from here on
  void moveTo(DevPool& to) {
    to.ptrs.insert(to.ptrs.end(), ptrs.begin(), ptrs.end());
    ptrs.clear();
  }
};

// Morph targets (bdpt_set_morph): the vertex-major entries, the active-vertex list, without a skin the base and the
// morphed streams, and the device weights (`weights`: where host-pointer weights are staged).
struct MorphState {
  DevPool allocs;
  bool have = false;
  MorphDev dev{};
  float* weights = nullptr;
};

// Skinning (bdpt_set_skin): the rest streams, weights, ids, the skinned streams and the device palettes (`palette`: where
// host-pointer palettes are staged: bones, normalBones).  A morph's base and outputs are its skin's, so it lives here.
struct SkinState {
  DevPool allocs;
  bool have = false;
  SkinDev dev{};
  float* palette[2] = {nullptr, nullptr};
  MorphState morph;
};

// The scene and what is derived from it on demand; every pointer below points into `allocs`.
struct SceneState {
  bool have = false;
  SceneDev S{};  // (its stackOvf / stackOvfStride are the context's: dropScene seeds them)
  DevPool allocs;
  bdpt_bvh_info bvhInfo{};
  uint32_t numVertices = 0, numTriangles = 0;
  // occluder hints of next-event rays: one cube map per light (= S.lightMap, writable).  BDPT_NO_HINTS (environment, read
  // by bdpt_set_scene and bdpt_resize) switches these and the frame's hintPix off.
  bool hints = true;
  uint32_t* lightMaps = nullptr;
  // refit (bdpt_update_geometry / bdpt_set_lights): the plan and its scratch, made on first use or by
  // bdpt_prepare(BDPT_PREPARE_REFIT)
  bool refitReady = false;
  BvhRefitPlan refitPlan;  // (host copy: the SAH of bdpt_get_refit_info walks it)
  RefitDev refit{};
  uint32_t numUpdates = 0;
  float* stage[3] = {nullptr, nullptr, nullptr};  // device copies of host-pointer inputs: positions, normals, bitangents
  bool stageInFlight = false;                     // the context's pinned buffer is still being read (evStage)
  // area lights (BDPT_PARAM_AREA_LIGHTS): the emitter table, made by bdpt_prepare(BDPT_PREPARE_AREA_LIGHTS) or the first
  // frame with the switch; refreshed on the device by every update.  alphaTris: the non-opaque triangles in ascending
  // order (their alpha-test records' order), kept for the table build.
  const uint32_t* alphaTris = nullptr;
  uint32_t numAlphaTris = 0;
  bool areaReady = false;
  AreaDev area{};
  uint32_t areaTextured = 0;
  float* areaBlockSum = nullptr;  // one float and one word per 64 emitters: the refresh's scratch
  uint32_t* areaBlockLast = nullptr;
  // motion (bdpt_prepare(BDPT_PREPARE_MOTION)): the previous pose, three float4 per primitive; bdpt_keep_pose copies the
  // current corners into it
  float4* prevPose = nullptr;
  SkinState skin;
};

// What the denoiser keeps between frames for `slots` images over one G-buffer: position / normal ping-pong pairs, accept
// and prevPixel once, noisy and filtered pairs per slot (side s of slot k at [(2 * k + s) * W * H]).  Own allocations:
// growing frees them (the history goes with the frame, BlockwiseMultiOrderFeatureRegression::resize).
struct BmfrHistory {
  float4* pos[2] = {nullptr, nullptr};
  float4* norm[2] = {nullptr, nullptr};
  float4 *noisy = nullptr, *filtered = nullptr;
  uint8_t* accept = nullptr;  // set: the history is allocated
  uint32_t* prevPixel = nullptr;
  uint32_t slots = 0;
  int read = 0;  // which side holds the previous frame
};

// The tile: which frame rows this context renders (a contiguous band, or the stripes of one owner) and where splat
// accumulators live (SplatLayout); rows in ascending order
struct TileDesc {
  std::vector<std::pair<uint32_t, uint32_t>> rowRanges;  // [first, last) runs of rows
  uint32_t rows = 0;
  SplatLayout sl{1, 1, 0};
  bdpt_stripes stripes{0, 1, 0};  // stripeRows == 0: contiguous band (bdpt_resize)
};

// The frame size and the workspaces sized by it; the pointers (but the histories') point into `allocs`.
struct FrameState {
  bool have = false;
  uint32_t W = 0, H = 0, maxDepth = 0;
  TileDesc tile;
  PathBuf P{};
  DevPool allocs;
  unsigned long long* splat = nullptr;  // buffer in use (own or caller-provided)
  unsigned long long* ownSplat = nullptr;
  DevCounters* counters = nullptr;
  int lazyRounds = 3;
  // channels of the built-in primary stage (bdpt_execute with in == NULL): bdpt_prepare or first use
  bdpt_gbuffer ownGb{};
  // occluder hints (kernels.hip "Occluder hints"): the primary-visibility triangle of every frame pixel, written by this
  // context's G-buffer pass and read by its light-tracing generator.  A context that renders only part of the frame fills
  // the hints of ALL frame pixels when its camera changes (its light-tracing rays aim anywhere); its own rows are
  // refreshed by every G-buffer pass.
  uint32_t* hintPix = nullptr;
  bdpt_camera hintCam{};
  bool hintCamValid = false;
  // BMFR history, two of them and apart: bmfr for bdpt_bmfr_execute / _motion (one slot; bdpt_prepare(BDPT_PREPARE_BMFR)
  // or the first call), bmfrPlanes for bdpt_bmfr_execute_planes (bdpt_bmfr_planes_prepare or the first call that needs
  // more slots)
  BmfrHistory bmfr, bmfrPlanes;
};

// Light groups (bdpt_execute_light_groups, bdpt_execute_grouped): the splat-value planes and each pixel's light, made by
// bdpt_prepare(BDPT_PREPARE_LIGHT_GROUPS / _LIGHT_GROUP_TABLE) or by the first call that needs more planes than there are.
struct LightGroups {
  unsigned long long* splat = nullptr;
  uint32_t planes = 0;
  uint8_t* lightIdx = nullptr;
};

// The sampling table of the environment map (bdpt_env_prepare): made for the map bdpt_set_environment bound, so that call
// drops it (dropEnv), as bdpt_destroy does.  The map itself stays the caller's.
struct EnvState {
  DevPool allocs;
  bool ready = false;
  EnvTable table{};             // the snapshot of the map, and cdf / rowCdf (in `allocs`)
  uint32_t* maxBits = nullptr;  // two words (in `allocs`): [0] the running maximum, zero between builds; [1] the bits of m
  uint64_t bytes = 0;           // what `allocs` holds
};
}  // namespace bdpt

struct bdpt_ctx {
  bdpt::SceneState scene;
  bdpt::FrameState frame;
  bdpt::LightGroups groups;
  bdpt::EnvState envTable;
  // ---- from bdpt_create to bdpt_destroy ----
  int device = 0;
  int numCUs = 256;
  std::string err;
  bool haveCamera = false;
  bdpt_camera cam{};
  bdpt_environment env{};  // bdpt_set_environment: what BDPT_PARAM_ENV_ON_MISS looks up (none: black)
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
  bdpt::LaunchGrids grids{};  // persistent-grid sizes for this context's device
  int* stackOvf = nullptr;      // overflow rows of the persistent kernels' traversal stacks (kernels.h kStackLds)
  uint32_t stackOvfStride = 0;  // lanes per row: every wave a persistent grid can hold
  unsigned long long* rayCursor = nullptr;  // fetch cursor and done count of bdpt_trace_rays (each launch leaves them zero)
  unsigned long long* adaptiveSum = nullptr;  // active-pixel sum and done count of bdpt_adaptive_update (each launch leaves them zero)
  // the splat and NEE generators run beside the connection generator on this stream (fork/join with events; capture-safe)
  hipStream_t walkStream = nullptr;
  hipEvent_t evFork = nullptr, evJoin = nullptr, evSplat = nullptr;
  // host-pointer inputs go through pinned memory (copied before the call returns); evStage marks the end of the copy
  // that last read it
  void* pinned = nullptr;
  size_t pinnedBytes = 0;
  hipEvent_t evStage = nullptr, evOrder = nullptr;
};
