// Passes.h — the three passes of the reference pipeline that sit on the hot path, with the
// reference's class names, factories and GUI-exposed state:
//   LightProbeGBufferPass   CommonPasses/LightProbeGBufferPass.{h,cpp}
//   BDPTPass                BidirectionalPathtracing/Passes/BDPTPass.{h,cpp}
//   SimpleAccumulationPass  CommonPasses/SimpleAccumulationPass.{h,cpp}
// the framework's ambient occlusion pass, AmbientOcclusionPass (CommonPasses/AmbientOcclusionPass.{h,cpp}),
// its one-bounce path tracer, SimpleDiffuseGIPass (CommonPasses/SimpleDiffuseGIPass.{h,cpp}),
// its direct lighting pass, LambertianPlusShadowPass (CommonPasses/LambertianPlusShadowPass.{h,cpp}),
// plus RayLaunch, the thin launch wrapper they hold (SharedUtils/RayLaunch.h:85-135): here it owns
// one bdpt_ctx and forwards to the C ABI of include/bdpt.h instead of building a DXR state object.
#pragma once
#include "../../include/bdpt.h"
#include "RenderPass.h"
#include "Tiling.h"

namespace bdpt {

// One bdpt_ctx shared by the passes of a pipeline (they trace the same scene on the same device).
class RayLaunch {
 public:
  using SharedPtr = std::shared_ptr<RayLaunch>;
  // All passes created for one device share the same launcher (and so the same BVH).
  static SharedPtr create(RenderContext* ctx);
  ~RayLaunch();
  void setScene(Scene::SharedPtr pScene);           // RayLaunch::setScene -> bdpt_set_scene (BVH build)
  // Animated scenes (RtScene::update -> the acceleration structure refitted in place, RtScene.cpp:74-83, 244-283):
  // the same update for every frame slot's context (each holds the scene), slot k on streams[k], in frame order from
  // slot `first`.  false + lastError() when a context refuses it.
  bool updateGeometry(const bdpt_geometry_update& u, const std::vector<hipStream_t>& streams, uint32_t first);
  bool setLights(const bdpt_light* lights, uint32_t numLights, const std::vector<hipStream_t>& streams, uint32_t first);
  // Skinning (SkinningCache::update in front of the refit): the same skin for every frame slot's context (synchronises;
  // nullptr drops it), and the same bone palette for each, ordered as updateGeometry's.
  bool setSkin(const bdpt_skin_desc* skin);
  bool updateSkinned(const bdpt_skin_update& u, const std::vector<hipStream_t>& streams, uint32_t first);
  // Motion (include/bdpt.h "Motion"): a pass that wants the PrevWorldPosition channel asks for the previous pose; every
  // frame slot's context then prepares it with its scene (bdpt_prepare(BDPT_PREPARE_MOTION)), and keepPose makes the
  // current pose the previous one on each, ordered as updateGeometry's.
  bool requestMotion();
  bool motion() const { return mMotion; }
  bool keepPose(const std::vector<hipStream_t>& streams, uint32_t first);
  // Piece-tight refit (include/bdpt.h "Animated scenes"): every frame slot's context prepares it with its scene
  // (bdpt_prepare(BDPT_PREPARE_REFIT_PIECES)), before the scene's first update; later updates then refit by pieces.
  bool requestTightRefit();
  void setMaxRecursionDepth(uint32_t d) { mMaxDepth = d; }
  bool readyToRender() const { return mCtx && mSceneSet; }
  // (re)size the per-pixel path state; called by execute when the screen size changed
  bool ensureSize(uint32_t w, uint32_t h);
  bdpt_ctx* ctx() const { return mSlot == 0 ? mCtx : mMore[mSlot - 1]; }
  Scene::SharedPtr scene() const { return mpScene; }
  const char* lastError() const;
  // Frames in flight: one bdpt_ctx per frame slot (each owns its path state and traverses its own copy of the BVH)
  bool setSlotCount(uint32_t n);
  void setCurrentSlot(uint32_t s) { mSlot = s <= mMore.size() ? s : 0; }
  uint32_t currentSlot() const { return mSlot; }
  // Multi-GPU tiling (Tiling.h): every context of this launcher renders the stripes of rank
  // x->rank() of x->world() (bdpt_resize_stripes) and keeps its splat accumulators owner-major; the passes then run the
  // two-phase execute with the exchange in between.  Call before the first frame (RenderingPipeline::setTiling does).
  void setTiling(TileExchange::SharedPtr x);
  bool tiled() const { return mExchange != nullptr; }
  TileExchange::SharedPtr exchange() const { return mExchange; }
  const bdpt_tile_info& tileInfo() const { return mTileInfo; }
  uint32_t stripeRows() const { return mStripeRows; }
  uint64_t* tileSplat() const { return mTileSplat.empty() ? nullptr : mTileSplat[mSlot]; }  // the current slot's reduced chunk

 private:
  RayLaunch() = default;
  void freeTileSplat();
  TileExchange::SharedPtr mExchange;
  bdpt_tile_info mTileInfo{};
  uint32_t mStripeRows = 0;
  std::vector<uint64_t*> mTileSplat;  // per slot: chunkU64 words, receives this rank's chunk of the reduce-scatter
  bdpt_ctx* mCtx = nullptr;
  std::vector<bdpt_ctx*> mMore;  // slots 1..
  uint32_t mSlot = 0;
  int mDevice = 0;
  Scene::SharedPtr mpScene;
  bool mSceneSet = false;
  bool mMotion = false;
  bool prepareMotion();
  bool mTightRefit = false;
  bool prepareTightRefit();
  uint32_t mW = 0, mH = 0, mMaxDepth = 8, mSizedDepth = 0;
};

class LightProbeGBufferPass : public RenderPass {
 public:
  using SharedPtr = std::shared_ptr<LightProbeGBufferPass>;
  static SharedPtr create() { return SharedPtr(new LightProbeGBufferPass()); }

 protected:
  LightProbeGBufferPass() : RenderPass("G-Buf With Light Probe", "G-Buffer With Light Probe Options") {}
  bool initialize(RenderContext* pRenderContext, ResourceManager::SharedPtr pResManager) override;
  void execute(RenderContext* pRenderContext) override;
  void renderGui(Gui* pGui) override;
  void initScene(RenderContext* pRenderContext, Scene::SharedPtr pScene) override;
  bool requiresScene() override { return true; }
  bool usesRayTracing() override { return true; }
  bool usesEnvironmentMap() override { return true; }

  RayLaunch::SharedPtr mpRays;
  Scene::SharedPtr mpScene;
  bool mUseThinLens = false;
  float mFStop = 32.0f, mFocalLength = 1.0f, mLensRadius = 0.0f;
  bool mUseJitter = true, mUseRandomJitter = false;  // random jitter (std::mt19937 seeded by time) is not reproduced
  void saveState(RenderContext* pRenderContext, std::vector<uint8_t>& out) override;
  bool loadState(RenderContext* pRenderContext, const uint8_t* data, size_t size) override;
  uint32_t mFrameCount = 0xdeadbeefu;
};

class BDPTPass : public RenderPass {
 public:
  using SharedPtr = std::shared_ptr<BDPTPass>;
  static SharedPtr create(const std::string& outChannel) { return SharedPtr(new BDPTPass(outChannel)); }
  // build-only switches (BDPT_PARAM_*), default 0 = reference behaviour
  void setParamFlags(uint32_t f) { mParamFlags = f; }

 protected:
  BDPTPass(const std::string& outChannel) : RenderPass("Bidirectional Pathtracer", "BDPT Options"), mOutputTextureName(outChannel) {}
  bool initialize(RenderContext* pRenderContext, ResourceManager::SharedPtr pResManager) override;
  void initScene(RenderContext* pRenderContext, Scene::SharedPtr pScene) override;
  void execute(RenderContext* pRenderContext) override;
  void renderGui(Gui* pGui) override;
  // The frame's path state is sized as soon as the frame size is known — before initScene builds the acceleration
  // structure, whose freed scratch the driver would otherwise have to clear again under these allocations
  void resize(uint32_t width, uint32_t height) override;
  bool requiresScene() override { return true; }
  bool usesRayTracing() override { return true; }

  RayLaunch::SharedPtr mpRays;
  Scene::SharedPtr mpScene;
  int32_t mUserSpecifiedRayDepth = 3;
  const int32_t mMaxPossibleRayDepth = 8;
  int32_t mMaterialIndex = 0;
  const int32_t mNumOfMaterials = 2;
  float mClampUpper = 0.9f;
  float mRefractiveIndex = 1.0f;
  std::string mOutputTextureName;
  void saveState(RenderContext* pRenderContext, std::vector<uint8_t>& out) override;
  bool loadState(RenderContext* pRenderContext, const uint8_t* data, size_t size) override;
  uint32_t mFrameCount = 0x1337u;
  uint32_t mParamFlags = 0;
};

class SimpleAccumulationPass : public RenderPass {
 public:
  using SharedPtr = std::shared_ptr<SimpleAccumulationPass>;
  static SharedPtr create(const std::string& bufferToAccumulate) { return SharedPtr(new SimpleAccumulationPass(bufferToAccumulate)); }
  uint32_t getAccumCount() const { return mAccumCount; }

 protected:
  SimpleAccumulationPass(const std::string& bufferToAccumulate) : RenderPass("Accumulation Pass", "Accumulation Options") {
    mAccumChannel = bufferToAccumulate;
  }
  bool initialize(RenderContext* pRenderContext, ResourceManager::SharedPtr pResManager) override;
  void initScene(RenderContext* pRenderContext, Scene::SharedPtr pScene) override;
  void execute(RenderContext* pRenderContext) override;
  void renderGui(Gui* pGui) override;
  void resize(uint32_t width, uint32_t height) override;
  void stateRefreshed() override;
  bool appliesPostprocess() override { return true; }
  bool hasAnimation() override { return false; }
  bool needsFrameOrder() override { return true; }  // the running mean is applied in frame order
  bool hasCameraMoved();
  void saveState(RenderContext* pRenderContext, std::vector<uint8_t>& out) override;
  bool loadState(RenderContext* pRenderContext, const uint8_t* data, size_t size) override;

  std::string mAccumChannel;
  RayLaunch::SharedPtr mpRays;  // only for the context that runs bdpt_accumulate
  Texture::SharedPtr mpLastFrame;
  Scene::SharedPtr mpScene;
  uint64_t mLastCameraVersion = 0;
  bool mDoAccumulation = true;
  bool mResumed = false;  // state came from a checkpoint: the next frame's camera set-up is not a camera move
  uint32_t mAccumCount = 0;
  int32_t mCountLimit = 100;
  const int32_t mMaxCountLimit = 10000;
};

// Ray traced ambient occlusion (CommonPasses/AmbientOcclusionPass.{h,cpp}): WorldPosition and WorldNormal in, the output
// channel out, the reference's GUI state and defaults.  Its ray generation shader is bdpt_ao_execute.
class AmbientOcclusionPass : public RenderPass {
 public:
  using SharedPtr = std::shared_ptr<AmbientOcclusionPass>;
  static SharedPtr create(const std::string& outBuf = ResourceManager::kOutputChannel) { return SharedPtr(new AmbientOcclusionPass(outBuf)); }

 protected:
  AmbientOcclusionPass(const std::string& outBuf) : RenderPass("Ambient Occlusion Rays", "Ambient Occlusion Options") { mOutputTexName = outBuf; }
  bool initialize(RenderContext* pRenderContext, ResourceManager::SharedPtr pResManager) override;
  void initScene(RenderContext* pRenderContext, Scene::SharedPtr pScene) override;
  void renderGui(Gui* pGui) override;
  void execute(RenderContext* pRenderContext) override;
  bool requiresScene() override { return true; }
  bool usesRayTracing() override { return true; }
  void saveState(RenderContext* pRenderContext, std::vector<uint8_t>& out) override;
  bool loadState(RenderContext* pRenderContext, const uint8_t* data, size_t size) override;

  RayLaunch::SharedPtr mpRays;
  Scene::SharedPtr mpScene;
  float mAORadius = 0.0f;        // AmbientOcclusionPass.h:53; initScene sets the scene's default
  uint32_t mFrameCount = 0;      // AmbientOcclusionPass.h:54
  int32_t mNumRaysPerPixel = 1;  // AmbientOcclusionPass.h:55
  int32_t mPositionIndex = -1, mNormalIndex = -1, mOutputIndex = -1;
  std::string mOutputTexName;
};

// One-bounce diffuse global illumination (CommonPasses/SimpleDiffuseGIPass.{h,cpp}): WorldPosition, WorldNormal, MaterialDiffuse
// and the environment map in, the output channel out, the reference's three switches and defaults.  Its ray generation
// shader with its hit groups is bdpt_gi_execute.
class SimpleDiffuseGIPass : public RenderPass {
 public:
  using SharedPtr = std::shared_ptr<SimpleDiffuseGIPass>;
  static SharedPtr create(const std::string& outBuf) { return SharedPtr(new SimpleDiffuseGIPass(outBuf)); }

 protected:
  SimpleDiffuseGIPass(const std::string& outBuf) : RenderPass("Simple Diffuse GI Ray", "Simple Diffuse GI Options"), mOutputBuf(outBuf) {}
  bool initialize(RenderContext* pRenderContext, ResourceManager::SharedPtr pResManager) override;
  void initScene(RenderContext* pRenderContext, Scene::SharedPtr pScene) override;
  void renderGui(Gui* pGui) override;
  void execute(RenderContext* pRenderContext) override;
  bool requiresScene() override { return true; }
  bool usesRayTracing() override { return true; }
  bool usesEnvironmentMap() override { return true; }
  void saveState(RenderContext* pRenderContext, std::vector<uint8_t>& out) override;
  bool loadState(RenderContext* pRenderContext, const uint8_t* data, size_t size) override;

  RayLaunch::SharedPtr mpRays;
  Scene::SharedPtr mpScene;
  std::string mOutputBuf;
  bool mDoIndirectGI = true;        // SimpleDiffuseGIPass.h:57
  bool mDoCosSampling = true;       // SimpleDiffuseGIPass.h:58
  bool mDoDirectShadows = true;     // SimpleDiffuseGIPass.h:59: sets gDirectShadow, which the shader does not declare
  uint32_t mFrameCount = 0x1337u;   // SimpleDiffuseGIPass.h:62
};

// Sky lighting: importance-sampled shadow rays toward the environment map (no pass of the reference: it is shaped like the
// AO pass above).  WorldPosition, WorldNormal, MaterialDiffuse and the environment map in, the output channel out.  The
// map's sampling table is prepared when the map bound to the pass's context changes.  Its kernel is bdpt_sky_execute; with
// MIS on it is bdpt_sky_mis_execute (a table-sampled and a BSDF-sampled ray per sample, balance heuristic), for the
// Lambertian surface or, with material 0, the pass's GGX material: MaterialSpecRough and the scene's camera then go in too.
// MIS and the material are the host program's configuration, like the clamp: the checkpoint record does not hold them.
class SkyLightingPass : public RenderPass {
 public:
  using SharedPtr = std::shared_ptr<SkyLightingPass>;
  static SharedPtr create(const std::string& outBuf = ResourceManager::kOutputChannel) { return SharedPtr(new SkyLightingPass(outBuf)); }
  void setClamp(float hi) { mClampUpper = hi; }
  void setMis(bool on) { mUseMis = on; }
  void setMaterial(int matIndex) { mMatIndex = matIndex; }  // 0 GGX (with MIS only), 1 Lambertian
  // The table is a snapshot of the map's contents, made again when the map's address or size changes.  A host that
  // rewrites the map in place calls this, and the next frame prepares the table anew.
  void environmentChanged() { mPreparedMap = nullptr; }

 protected:
  SkyLightingPass(const std::string& outBuf) : RenderPass("Sky Lighting Rays", "Sky Lighting Options"), mOutputBuf(outBuf) {}
  bool initialize(RenderContext* pRenderContext, ResourceManager::SharedPtr pResManager) override;
  void initScene(RenderContext* pRenderContext, Scene::SharedPtr pScene) override;
  void renderGui(Gui* pGui) override;
  void execute(RenderContext* pRenderContext) override;
  bool requiresScene() override { return true; }
  bool usesRayTracing() override { return true; }
  bool usesEnvironmentMap() override { return true; }
  void saveState(RenderContext* pRenderContext, std::vector<uint8_t>& out) override;
  bool loadState(RenderContext* pRenderContext, const uint8_t* data, size_t size) override;

  RayLaunch::SharedPtr mpRays;
  Scene::SharedPtr mpScene;
  std::string mOutputBuf;
  float mClampUpper = 3.402823466e+38f;  // no clamp
  bool mUseMis = false;
  int32_t mMatIndex = 1;
  uint32_t mFrameCount = 0;
  int32_t mNumRaysPerPixel = 1;
  const float* mPreparedMap = nullptr;  // the map the context's table was made for, and its size
  uint32_t mPreparedW = 0, mPreparedH = 0;
};

// Resampled direct lighting (include/bdpt.h "Resampled direct lighting"): WorldPosition, WorldNormal and MaterialDiffuse in, the
// output channel out; per pixel and sample `candidates` next-event candidates, one survivor, one shadow ray: bdpt_ris_execute.
// The project's own pass, shaped like SkyLightingPass: a frame counter from 0, one per frame, so that an accumulation pass
// behind it converges.  Material 0 is the pass's GGX material (MaterialSpecRough and the scene's camera go in too); the
// emitter table, the occluder hints and the clamp are the host program's configuration.
class ResampledDirectPass : public RenderPass {
 public:
  using SharedPtr = std::shared_ptr<ResampledDirectPass>;
  static SharedPtr create(const std::string& outBuf = ResourceManager::kOutputChannel) { return SharedPtr(new ResampledDirectPass(outBuf)); }
  void setCandidates(int m) { mCandidates = m; }   // 1 .. BDPT_RIS_MAX_CANDIDATES
  void setSamples(int k) { mSamples = k; }          // 1 .. BDPT_RIS_MAX_SAMPLES
  void setMaterial(int matIndex) { mMatIndex = matIndex; }  // 0 GGX, 1 Lambertian
  void setAreaLights(bool on) { mAreaLights = on; }
  void setHints(bool on) { mUseHints = on; }
  void setClamp(float hi) { mClampUpper = hi; }

 protected:
  ResampledDirectPass(const std::string& outBuf) : RenderPass("Resampled Direct Rays", "Resampled Direct Options"), mOutputBuf(outBuf) {}
  bool initialize(RenderContext* pRenderContext, ResourceManager::SharedPtr pResManager) override;
  void initScene(RenderContext* pRenderContext, Scene::SharedPtr pScene) override;
  void renderGui(Gui* pGui) override;
  void execute(RenderContext* pRenderContext) override;
  bool requiresScene() override { return true; }
  bool usesRayTracing() override { return true; }
  void saveState(RenderContext* pRenderContext, std::vector<uint8_t>& out) override;
  bool loadState(RenderContext* pRenderContext, const uint8_t* data, size_t size) override;

  RayLaunch::SharedPtr mpRays;
  Scene::SharedPtr mpScene;
  std::string mOutputBuf;
  float mClampUpper = 3.402823466e+38f;  // no clamp
  int32_t mCandidates = 8;
  int32_t mSamples = 1;
  int32_t mMatIndex = 1;
  bool mAreaLights = false;
  bool mUseHints = false;
  uint32_t mFrameCount = 0;
};

// ReSTIR direct lighting (include/bdpt.h "Reservoir reuse"): the resampled pass with one sample and its reservoirs
// (bdpt_ris_execute_reservoirs), then with setTemporal and a history a bdpt_reuse_execute whose one neighbour is the same pixel
// of last frame's reservoirs, G-buffer copy and camera position, then with setSpatial(N > 0) a bdpt_reuse_execute over N
// neighbours at offsets drawn within the radius; one shadow ray per pixel and pass.  The first stage runs at the pass's frame
// counter (from 0), the temporal pass at twice it, the spatial pass at twice plus one: FramePipeline.restir_lighting of the
// Python package is the same sequence, bit for bit.  The last pass's image is the frame — the history is the accumulation, no
// accumulation pass follows — and its reservoirs, the G-buffer and the camera position are the next frame's history, which a
// scene move (stateRefreshed) drops and a checkpoint carries.
class RestirDirectPass : public RenderPass {
 public:
  using SharedPtr = std::shared_ptr<RestirDirectPass>;
  static SharedPtr create(const std::string& outBuf = ResourceManager::kOutputChannel) { return SharedPtr(new RestirDirectPass(outBuf)); }
  void setCandidates(int m) { mCandidates = m; }  // 1 .. BDPT_RIS_MAX_CANDIDATES
  void setSpatial(int n) { mSpatial = n; }        // 0 .. BDPT_REUSE_MAX_NEIGHBORS
  void setRadius(int r) { mRadius = r; }          // 1 .. BDPT_REUSE_MAX_RADIUS
  void setTemporal(bool on) { mTemporal = on; }
  void setMaxM(int c) { mMaxM = c; }              // what a pool reservoir counts for at most; <= 0: 20 * candidates
  void setMaterial(int matIndex) { mMatIndex = matIndex; }  // 0 GGX, 1 Lambertian
  void setAreaLights(bool on) { mAreaLights = on; }
  void setClamp(float hi) { mClampUpper = hi; }

 protected:
  RestirDirectPass(const std::string& outBuf) : RenderPass("ReSTIR Direct Rays", "ReSTIR Direct Options"), mOutputBuf(outBuf) {}
  bool initialize(RenderContext* pRenderContext, ResourceManager::SharedPtr pResManager) override;
  void initScene(RenderContext* pRenderContext, Scene::SharedPtr pScene) override;
  void execute(RenderContext* pRenderContext) override;
  void stateRefreshed() override { mHistoryValid = false; }  // other lights or geometry: the history's samples are stale
  void resize(uint32_t width, uint32_t height) override { mW = width, mH = height, mHistoryValid = false; }
  bool requiresScene() override { return true; }
  bool usesRayTracing() override { return true; }
  bool holdsTemporalState() override { return true; }
  void saveState(RenderContext* pRenderContext, std::vector<uint8_t>& out) override;
  bool loadState(RenderContext* pRenderContext, const uint8_t* data, size_t size) override;
  bool ensureBuffers(uint32_t w, uint32_t h);
  uint32_t maxM() const { return mMaxM > 0 ? (uint32_t)mMaxM : 20u * (uint32_t)mCandidates; }
  uint32_t settingsWord() const;

  RayLaunch::SharedPtr mpRays;
  Scene::SharedPtr mpScene;
  std::string mOutputBuf;
  float mClampUpper = 3.402823466e+38f;  // no clamp
  float mNormalMin = 0.9f;               // a neighbour's rejection test, FramePipeline.restir_lighting's default (no plane test)
  int32_t mCandidates = 8, mSpatial = 0, mRadius = 8, mMaxM = 0, mMatIndex = 1;
  bool mTemporal = false, mAreaLights = false;
  uint32_t mFrameCount = 0;
  // reservoir images (RGBA32F-sized: 16 bytes a record): the history and one per pass; the history's G-buffer copy
  Texture::SharedPtr mHist, mFirst, mSecond, mThird, mHistPos, mHistNrm, mHistDif, mHistSpec;
  float mHistCam[3] = {0.0f, 0.0f, 0.0f};
  uint32_t mW = 0, mH = 0;  // the frame, as resize() last said
  uint32_t mHistM = 0;  // the candidate count of every history record; 0: the records' M words (a reuse pass wrote them)
  bool mHistoryValid = false;
};

// Direct lighting from every light with one shadow ray each (CommonPasses/LambertianPlusShadowPass.{h,cpp}): WorldPosition,
// WorldNormal, MaterialDiffuse and MaterialSpecRough in, the output channel out; no GUI state and no frame counter, as in the
// reference (nothing is drawn).  Its ray generation shader with its shadow hit group is bdpt_direct_execute.
class LambertianPlusShadowPass : public RenderPass {
 public:
  using SharedPtr = std::shared_ptr<LambertianPlusShadowPass>;
  static SharedPtr create() { return SharedPtr(new LambertianPlusShadowPass()); }
  // BDPT_DIRECT_USE_HINTS: the lights' occluder hints are tried before a traversal (the same image); not in the reference
  void setUseHints(bool on) { mUseHints = on; }

 protected:
  LambertianPlusShadowPass() : RenderPass("Lambertian Plus Shadows", "Lambertian Plus Shadow Options") {}
  bool initialize(RenderContext* pRenderContext, ResourceManager::SharedPtr pResManager) override;
  void initScene(RenderContext* pRenderContext, Scene::SharedPtr pScene) override;
  void execute(RenderContext* pRenderContext) override;
  bool requiresScene() override { return true; }
  bool usesRayTracing() override { return true; }
  void saveState(RenderContext* pRenderContext, std::vector<uint8_t>& out) override;
  bool loadState(RenderContext* pRenderContext, const uint8_t* data, size_t size) override;

  RayLaunch::SharedPtr mpRays;
  Scene::SharedPtr mpScene;
  bool mUseHints = false;
};

// BMFR denoiser pass (BidirectionalPathtracing/Passes/DenoisePass.{h,cpp}): same channels, switches and defaults
// (off until "Do BMFR Denoise" is ticked; regression off, pre/post-process on, DenoisePass.h:70-75).  The three
// shaders and their history textures live behind bdpt_bmfr_execute.
class BlockwiseMultiOrderFeatureRegression : public RenderPass {
 public:
  using SharedPtr = std::shared_ptr<BlockwiseMultiOrderFeatureRegression>;
  static SharedPtr create(const std::string& bufferToDenoise = ResourceManager::kOutputChannel) {
    return SharedPtr(new BlockwiseMultiOrderFeatureRegression(bufferToDenoise));
  }
  uint32_t getAccumCount() const { return mAccumCount; }
  // Motion-aware reprojection for animated scenes (bdpt_bmfr_execute_motion): the pass requests the PrevWorldPosition
  // channel, which the G-buffer pass then renders, and the pipeline keeps the previous pose once per frame.  Call before
  // the pipeline's initialize().  Whole-frame pipelines only: a tiled pipeline runs the plain call (the channel is not
  // part of its all-gather).  Default off: the reference's static-scene behaviour.
  void setMotion(bool on) { mMotion = on; }
  ~BlockwiseMultiOrderFeatureRegression() override { freeGather(); }

 protected:
  BlockwiseMultiOrderFeatureRegression(const std::string& bufferToDenoise) : RenderPass("BMFR Denoise Pass", "BMFR Denoise Options") {
    mDenoiseChannel = bufferToDenoise;
  }
  bool initialize(RenderContext* pRenderContext, ResourceManager::SharedPtr pResManager) override;
  void initScene(RenderContext* pRenderContext, Scene::SharedPtr pScene) override;
  void execute(RenderContext* pRenderContext) override;
  void renderGui(Gui* pGui) override;
  void resize(uint32_t width, uint32_t height) override;
  bool appliesPostprocess() override { return true; }
  bool hasAnimation() override { return false; }
  // The temporal history (previous position / normal / noisy / filtered frames) lives inside the launcher context: frames
  // run one by one while the denoiser is on, and a checkpoint carries the history (bdpt_bmfr_save_history) beside the
  // frame number.
  bool holdsTemporalState() override { return mDoDenoise; }
  void saveState(RenderContext* pRenderContext, std::vector<uint8_t>& out) override;
  bool loadState(RenderContext* pRenderContext, const uint8_t* data, size_t size) override;
  // Tiled (RenderingPipeline::setTiling): the filter's blocks need their neighbours, so every rank gathers the WHOLE
  // noisy frame and the three feature channels (its rows packed, one all-gather, the rows put back) and filters the
  // same whole frame; the result replaces the rank's output channel, all rows of it.
  bool gatherWholeFrame(RenderContext* pRenderContext, Texture::SharedPtr noisy, Texture::SharedPtr pos, Texture::SharedPtr nrm, Texture::SharedPtr alb);
  void freeGather();

  std::string mDenoiseChannel;
  RayLaunch::SharedPtr mpRays;
  Scene::SharedPtr mpScene;
  bool mDoDenoise = false;
  bool mBMFR_preprocess = true;
  bool mBMFR_postprocess = true;
  bool mBMFR_regression = false;
  bool mBMFR_removeFeatures = true;
  bool mMotion = false;
  uint32_t mAccumCount = 0;
  // tiled: this rank's packed rows of the four channels, all ranks' (after the all-gather), and the whole-frame copies
  uint8_t *mPackedMine = nullptr, *mPackedAll = nullptr;
  float *mFullNoisy = nullptr, *mFullPos = nullptr;
  uint16_t *mFullNorm = nullptr, *mFullAlb = nullptr;
  uint32_t mGatherW = 0, mGatherH = 0;
};

// Headless counterpart of SharedUtils/RenderingPipeline (setPass + per-frame loop,
// RenderingPipeline.cpp:421-471, 611-695); the window, GUI rendering and final blit are out of scope.
class RenderingPipeline {
 public:
  RenderingPipeline();  // as Main.cpp:12 constructs it; the size comes with run()'s SampleConfig or with setSize()
  RenderingPipeline(uint32_t width, uint32_t height, int device = 0);
  ~RenderingPipeline();
  void setSize(uint32_t width, uint32_t height, int device = 0);  // before initialize()
  // Offline accumulation runs (a 1024-sample image is a long job; the reference's loop is interactive,
  // RenderingPipeline.cpp:611-695): keep n frames in flight, each on its own stream with its own channels and
  // launcher context, the ordered passes (accumulation) chained by events.  Same image as n = 1, bit for bit.
  // Call before initialize(); ignored (n = 1) while a pass holds temporal state of its own (the denoiser switched on).
  void setFramesInFlight(uint32_t n) { mFramesInFlight = n < 1 ? 1 : (n > 8 ? 8 : n); }
  uint32_t getFramesInFlight() const { return mFramesInFlight; }
  // Multi-GPU: this pipeline is rank `rank` of `world` pipelines (one per GPU, in threads of one process or in
  // processes of their own) that render ONE frame together — interleaved stripes of rows, scene replicated, splat
  // accumulators summed with one ncclReduceScatter per frame, the frame assembled by ncclAllGather when it is read
  // back (readOutput).  `comm` is this rank's RCCL communicator, created and destroyed by the host program; nullptr is
  // allowed for world == 1 (the tiled code path without a collective).  Call before initialize().  The passes and
  // their per-frame order (SharedUtils/RenderingPipeline.cpp:611-695) are unchanged; what is replaced is the single
  // DispatchRays of the reference (Falcor API/D3D12/D3D12RenderContext.cpp:350-384).  Same image as one GPU, bit for bit.
  bool setTiling(uint32_t rank, uint32_t world, ncclComm_t comm);
  // what TileExchange::abort calls instead of ncclCommAbort when this rank has to leave a collective (before initialize())
  void setTilingAbortHandler(std::function<void()> f) { mTileAbort = std::move(f); }
  bool isTiled() const { return mTileWorld > 0; }
  // RenderingPipeline::run (RenderingPipeline.cpp:697-712) without a window: size the channels from the config,
  // load the scene named by BDPT_SCENE (a .fscene / .obj path, "atrium", default the Cornell box), render BDPT_FRAMES
  // frames (default 1), and delete the pipeline.
  static void run(RenderingPipeline* pipe, SampleConfig& config);
  void setPass(uint32_t passNum, RenderPass::SharedPtr pTargetPass);
  // onLoad (initialize every pass, drop those that fail), onFirstRun (scene), onResize
  bool initialize(Scene::SharedPtr pScene);
  void renderFrame();                 // onFrameRender: refresh notifications, then every pass in order
  void applyGui(Gui* pGui);           // renderGui of every pass (scripted widget values)
  ResourceManager::SharedPtr getResourceManager() { return mpResourceManager; }
  RenderContext* getRenderContext() { return &mContext; }
  std::vector<float> readOutput();    // "PipelineOutput" as RGBA32F
  // every pass's cross-frame state (frame counters, accumulated frame) to / from a file: a run resumed from a
  // checkpoint continues the frame sequence bit for bit.  false on I/O errors, when a pass holds cross-frame state it
  // cannot serialise (the BMFR denoiser when switched on), or for a file that does not match this pipeline: other
  // passes, frame size, scene, or pass settings (ray depth, material model, clamp, lens, accumulation limit).  After a
  // failed load the pipeline's state is unspecified: discard it.
  bool saveCheckpoint(const std::string& path);
  bool loadCheckpoint(const std::string& path);
  // Animated scenes: new vertex positions (numVertices x 3; normals / bitangents may be null = unchanged) or moved
  // lights (the scene's count) for every frame slot, each on its slot's stream, in frame order; every rank of a tiled
  // pipeline applies the same update (the refit is deterministic: the replicas stay identical).  The next frame
  // restarts the accumulation (the refresh notification a camera move gives).  `memory`: BDPT_MEMORY_HOST / _DEVICE.
  // Checkpoints describe the scene as loaded: saveCheckpoint refuses after an update.
  bool updateGeometry(const float* positions, const float* normals = nullptr, const float* bitangents = nullptr,
                      uint32_t memory = BDPT_MEMORY_HOST, bool keepLightMaps = false);
  bool setLights(const bdpt_light* lights, uint32_t numLights);
  // Skinned scenes: setSkin hands every frame slot's context the rest pose, bone weights and ids (host arrays, copied;
  // call it after initialize(), it synchronises); updateSkinned then poses the scene from a bone palette (numBones x 16
  // floats, and the inverse transposes when the skin has normals) instead of three vertex streams — skinned on the
  // device, then refitted as by updateGeometry.  nullptr drops the skin.
  bool setSkin(const bdpt_skin_desc* skin);
  bool updateSkinned(const float* bones, const float* normalBones, uint32_t numBones, uint32_t memory = BDPT_MEMORY_HOST,
                     bool keepLightMaps = false);
  // Opt-in: split and alpha-clipped references are refitted by their piece instead of by their whole triangle (a tree that
  // stays close to its built quality under updateGeometry / updateSkinned).  Call it after initialize() and before the
  // scene's first update; it synchronises.
  bool setTightRefit();
  Scene::SharedPtr getScene() const { return mpScene; }
  size_t getPassCount() const { return mActivePasses.size(); }

 private:
  uint64_t sceneIdentity() const;
  RenderContext mContext;
  uint32_t mWidth, mHeight;
  ResourceManager::SharedPtr mpResourceManager;
  std::vector<RenderPass::SharedPtr> mActivePasses;
  Scene::SharedPtr mpScene;
  uint32_t mFramesInFlight = 1;
  uint64_t mFrameIndex = 0;
  std::vector<hipStream_t> mSlotStreams;   // one per frame slot (slot 0 included)
  std::vector<hipEvent_t> mOrderEvents;    // per ordered pass: recorded after it ran for the latest frame
  RayLaunch::SharedPtr mpRays;             // kept to switch the launcher's slot
  bool inFlightActive();
  std::vector<hipStream_t> updateStreams(uint32_t& first);
  void keepPose();
  bool mSceneMoved = false;    // the next frame delivers the refresh notification
  bool mSceneUpdated = false;  // since initialize(): no checkpoint
  uint32_t mTileRank = 0, mTileWorld = 0;  // world 0: not tiled
  std::function<void()> mTileAbort;
  ncclComm_t mTileComm = nullptr;
  std::string rankPath(const std::string& path) const;  // checkpoints of a tiled pipeline are per rank
};

}  // namespace bdpt
