// main.cpp — headless counterpart of BidirectionalPathtracing/Main.cpp:9-29: the same pipeline
// (G-buffer pass -> BDPT pass -> accumulation pass -> BMFR denoiser, which is off unless --denoise /
// --denoise-regression tick its boxes), run for a number of frames, output written as a PFM image.
// `--ao N` runs the G-buffer pass and the ambient occlusion pass instead (CommonPasses/AmbientOcclusionPass.cpp) and
// writes the AO channel; `--sky N` (with `--env FILE`) runs the G-buffer pass, the sky lighting pass and the accumulation pass;
// `--gi` runs the G-buffer pass, the one-bounce diffuse GI pass (CommonPasses/SimpleDiffuseGIPass.cpp)
// and the accumulation pass, so that --frames N converges; `--direct` runs the G-buffer pass and the direct lighting pass
// (CommonPasses/LambertianPlusShadowPass.cpp: every light, one shadow ray each, no draw) and writes its image.
//
// Multi-GPU: `--gpus N` runs N such pipelines, one per GPU, each on a host thread of its own
// with its own RCCL communicator (ncclCommInitAll); `--rank R --world N --id-file F` is the same for one PROCESS per
// GPU (ncclCommInitRank; rank 0 hands the ncclUniqueId to the others through file F).  Every rank renders its
// interleaved stripes of the ONE frame (RenderingPipeline::setTiling), the splat accumulators are summed with one
// ncclReduceScatter per frame, the frame is assembled with ncclAllGather when it is written.  `--gpus 1` takes the
// same code path through a one-rank communicator.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>

#include "RankSync.h"        // RankGroup: barrier + agreement point of the ranks of one process; the id-file protocol
#include "ReferenceNames.h"  // the mirror's classes under the reference's global names: no `using namespace`

static void writePfm(const char* path, const std::vector<float>& rgba, uint32_t w, uint32_t h) {
  FILE* f = std::fopen(path, "wb");
  if (!f) return;
  std::fprintf(f, "PF\n%u %u\n-1.0\n", w, h);
  for (int y = (int)h - 1; y >= 0; y--)  // PFM rows go bottom to top
    for (uint32_t x = 0; x < w; x++) std::fwrite(&rgba[((size_t)y * w + x) * 4], 4, 3, f);
  std::fclose(f);
}


namespace {
struct Options {
  std::string scene = "cornell", out = "bdpt_out.pfm", raw, checkpoint, resume, envFile, idFile, jobId;
  uint32_t W = 1280, H = 720;  // the reference's window, Main.cpp:23-24
  int frames = 8, depth = 3, mat = 0, device = 0, accumLimit = 100, inflight = 1, warmup = 0;
  int gpus = 0, rank = -1, world = 0;  // gpus: ranks as threads of this process; rank / world: this process is one rank
  bool denoise = false, denoiseRegression = false;
  bool areaLights = false;  // BDPT_PARAM_AREA_LIGHTS: emissive triangles light the scene (NEE and light subpaths)
  float sway = 0.0f;  // > 0: an animated scene — before every frame the vertices move by up to this fraction of the scene's extent
  bool noMotion = false;  // --sway / --bend with --denoise: keep the denoiser's static-scene reprojection (for comparison)
  bool tightRefit = false;  // --sway / --bend: refit split and alpha-clipped references by their piece (BDPT_PREPARE_REFIT_PIECES)
  int ao = -1;             // --ao N: render the G-buffer and the ambient occlusion pass (N rays per pixel) instead of the BDPT pipeline
  float aoRadius = 0.0f;   // --ao-radius R (with --ao, > 0); not given: the pass's default for the scene
  bool aoRadiusSet = false;
  int sky = -1;               // --sky N: render the G-buffer, the sky lighting pass (N rays per pixel) and the accumulation pass; needs --env
  float skyClamp = 0.0f;      // --sky-clamp C (with --sky, > 0): the bound of a sample's value; not given: none
  bool skyClampSet = false;
  bool skyMis = false;        // --sky-mis (with --sky): a table-sampled and a BSDF-sampled ray per sample, balance heuristic
  int ris = -1;               // --ris M: G-buffer -> ResampledDirectPass (M candidates per sample) -> accumulation
  int risSamples = 1;         // --ris-samples K (with --ris): shadow rays per pixel and frame
  bool risSamplesSet = false;
  bool risGgx = false;        // --ris-ggx (with --ris): the pass's GGX material instead of the Lambertian surface
  bool risHints = false;      // --ris-hints (with --ris): BDPT_RIS_USE_HINTS (the same image)
  float risClamp = 0.0f;      // --ris-clamp C (with --ris, > 0): the bound of a candidate's value; not given: none
  bool risClampSet = false;
  int risSpatial = 0;         // --ris-spatial N (with --ris): ReSTIR — N spatial neighbours behind the first stage (RestirDirectPass)
  int risRadius = 8;          // --ris-radius R (with --ris-spatial): the neighbours' offsets are drawn within R pixels
  bool risRadiusSet = false;
  bool risTemporal = false;   // --ris-temporal (with --ris): ReSTIR — the same pixel of last frame's reservoirs is a neighbour
  int risMaxM = 0;            // --ris-max-m C (with --ris-spatial / --ris-temporal): what a pool reservoir counts for at most; not given: 20 M
  bool risMaxMSet = false;
  bool restir() const { return ris >= 0 && (risSpatial > 0 || risTemporal); }
  bool skyGgx = false;        // --sky-ggx (with --sky-mis): the pass's GGX material instead of the Lambertian surface
  bool gi = false;            // --gi: render the G-buffer, the diffuse GI pass and the accumulation pass instead of the BDPT pipeline
  bool giDirectOnly = false;  // --gi-direct-only: untick "Shooting global illumination rays"
  bool giUniform = false;     // --gi-uniform: untick "Use cosine sampling"
  bool direct = false;       // --direct: render the G-buffer and the direct lighting pass (every light, one shadow ray each) instead of the BDPT pipeline
  bool directHints = false;  // --direct-hints: the lights' occluder hints are tried before a traversal (the same image)
  float bend = 0.0f;  // > 0: a skinned scene — a small rig along the scene's height, bent by up to this angle (radians) before every frame
};

// How the ranks of a job stay together: a rank whose set-up fails must not leave its peers waiting in a
// barrier or a collective it never enters.  Ranks as threads: bdpt::RankGroup (agreement point after set-up; abort() from
// a rank that fails later, upon which main()'s watcher calls ncclCommAbort on every communicator so that collectives in
// flight return).  One process per rank: the agreement is an ncclAllReduce(min) of an ok flag, and a rank that fails
// later aborts its own communicator and exits non-zero.
struct RankEnv {
  bdpt::RankGroup* group = nullptr;  // ranks as threads of this process (null: one rank per process, or the plain run)
  ncclComm_t comm = nullptr;
  uint32_t rank = 0, world = 0;
  // BDPT_RENDER_INJECT_FAILURE="<rank>:setup" | "<rank>:readback" (tests): that rank behaves as if the step had failed
  bool injected(const char* stage) const {
    const char* e = std::getenv("BDPT_RENDER_INJECT_FAILURE");
    if (!e) return false;
    const std::string want = std::to_string(rank) + ":" + stage;
    return want == e;
  }
  // every rank reports how its set-up went; true only if all went well
  bool agree(bool ok) const {
    if (group) return group->agree(ok);
    if (world <= 1 || !comm) return ok;
    int* flag = nullptr;
    int mine = ok ? 1 : 0, all = 0;
    if (hipMalloc(reinterpret_cast<void**>(&flag), sizeof(int)) != hipSuccess) {
      ncclCommAbort(comm);  // cannot even take part: the peers' all-reduce must not wait for this rank
      return false;
    }
    bool done = hipMemcpy(flag, &mine, sizeof(int), hipMemcpyHostToDevice) == hipSuccess &&
                ncclAllReduce(flag, flag, 1, ncclInt32, ncclMin, comm, nullptr) == ncclSuccess && hipStreamSynchronize(nullptr) == hipSuccess &&
                hipMemcpy(&all, flag, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(flag);
    return done && all == 1;
  }
  bool barrier() const { return group ? group->wait() : true; }
  // a failure after the agreement point
  void failLate() const {
    if (group) {
      group->abort();  // (idempotent; the watcher aborts every communicator once)
    } else if (comm && world > 1) {
      static std::atomic<bool> once{false};  // one rank per process: its one communicator is aborted once
      if (!once.exchange(true)) ncclCommAbort(comm);
    }
  }
};

struct RankResult {
  int rc = 1;
  double ms = 0;
};

Scene::SharedPtr makeScene(const Options& o, std::string* err) {
  // a path (.fscene / .obj) goes through the loader, as SceneLoaderWrapper::loadScene does for the file dialog's pick
  if (o.scene.find('.') != std::string::npos) return Scene::loadFromFile(o.scene, err);
  return o.scene == "atrium" ? Scene::createAtrium(1, 262144) : Scene::createCornellBox();
}

// set-up of one rank's pipeline; false (with a message) when any step fails
bool setUpRank(const Options& o, int device, uint32_t rank, uint32_t world, ncclComm_t comm, RenderingPipeline* pipeline) {
  const bool tiled = world > 0;
  std::string err;
  Scene::SharedPtr pScene = makeScene(o, &err);  // every rank holds the scene (and builds its BVH): replicated
  if (!pScene) {
    std::fprintf(stderr, "bdpt_render: %s\n", err.c_str());
    return false;
  }
  // add the passes to the rendering pipeline, as Main.cpp:12-18 does
  pipeline->setPass(0, LightProbeGBufferPass::create());
  const size_t numPasses = (o.ao >= 0 || o.direct || o.restir()) ? 2 : (o.gi || o.sky >= 0 || o.ris >= 0) ? 3 : 4;
  if (o.direct) {  // --direct: the G-buffer and the direct lighting pass, which writes the output channel (nothing to accumulate: no draw)
    LambertianPlusShadowPass::SharedPtr lambert = LambertianPlusShadowPass::create();
    lambert->setUseHints(o.directHints);
    pipeline->setPass(1, lambert);
  } else if (o.ao >= 0) {  // --ao: the G-buffer and the ambient occlusion pass, which writes the output channel
    pipeline->setPass(1, AmbientOcclusionPass::create(ResourceManager::kOutputChannel));
  } else if (o.sky >= 0) {  // --sky: the G-buffer, the sky lighting pass into the output channel, and the accumulation pass over it
    SkyLightingPass::SharedPtr sky = SkyLightingPass::create(ResourceManager::kOutputChannel);
    if (o.skyClampSet) sky->setClamp(o.skyClamp);
    sky->setMis(o.skyMis);
    sky->setMaterial(o.skyGgx ? 0 : 1);
    pipeline->setPass(1, sky);
    pipeline->setPass(2, SimpleAccumulationPass::create(ResourceManager::kOutputChannel));
  } else if (o.restir()) {  // --ris with reuse: the G-buffer and the ReSTIR pass, which writes the output channel (its history accumulates)
    RestirDirectPass::SharedPtr restir = RestirDirectPass::create(ResourceManager::kOutputChannel);
    restir->setCandidates(o.ris);
    restir->setSpatial(o.risSpatial);
    restir->setRadius(o.risRadius);
    restir->setTemporal(o.risTemporal);
    if (o.risMaxMSet) restir->setMaxM(o.risMaxM);
    restir->setMaterial(o.risGgx ? 0 : 1);
    restir->setAreaLights(o.areaLights);
    if (o.risClampSet) restir->setClamp(o.risClamp);
    pipeline->setPass(1, restir);
  } else if (o.ris >= 0) {  // --ris: the G-buffer, the resampled direct lighting pass into the output channel, the accumulation pass
    ResampledDirectPass::SharedPtr ris = ResampledDirectPass::create(ResourceManager::kOutputChannel);
    ris->setCandidates(o.ris);
    ris->setSamples(o.risSamples);
    ris->setMaterial(o.risGgx ? 0 : 1);
    ris->setAreaLights(o.areaLights);
    ris->setHints(o.risHints);
    if (o.risClampSet) ris->setClamp(o.risClamp);
    pipeline->setPass(1, ris);
    pipeline->setPass(2, SimpleAccumulationPass::create(ResourceManager::kOutputChannel));
  } else if (o.gi) {  // --gi: the G-buffer, the diffuse GI pass into the output channel, and the accumulation pass over it
    pipeline->setPass(1, SimpleDiffuseGIPass::create(ResourceManager::kOutputChannel));
    pipeline->setPass(2, SimpleAccumulationPass::create(ResourceManager::kOutputChannel));
  } else {
    BDPTPass::SharedPtr bdpt = BDPTPass::create(ResourceManager::kOutputChannel);
    if (o.areaLights) bdpt->setParamFlags(BDPT_PARAM_AREA_LIGHTS);
    pipeline->setPass(1, bdpt);
    pipeline->setPass(2, SimpleAccumulationPass::create(ResourceManager::kOutputChannel));
    BlockwiseMultiOrderFeatureRegression::SharedPtr bmfr = BlockwiseMultiOrderFeatureRegression::create();
    // an animated scene under the denoiser: reproject through the previous pose (whole-frame pipelines)
    bmfr->setMotion(o.denoise && (o.sway > 0.0f || o.bend > 0.0f) && !o.noMotion && !tiled);
    pipeline->setPass(3, bmfr);
  }
  // the window parameters of Main.cpp:20-25 size the channels (there is no window)
  SampleConfig config;
  config.windowDesc.resizableWindow = true;
  config.windowDesc.width = o.W;
  config.windowDesc.height = o.H;
  config.windowDesc.title = "Bidirectional Path Tracing (headless)";
  pipeline->setSize(config.windowDesc.width, config.windowDesc.height, device);
  pipeline->setFramesInFlight((uint32_t)(o.inflight < 1 ? 1 : o.inflight));  // offline accumulation: frames overlap, same image
  if (tiled && !pipeline->setTiling(rank, world, comm)) {
    std::fprintf(stderr, "bdpt_render: bad tiling (rank %u of %u)\n", rank, world);
    return false;
  }
  if (!pipeline->initialize(pScene) || pipeline->getPassCount() != numPasses) {
    std::fprintf(stderr, "pipeline initialisation failed (no GPU?)\n");
    return false;
  }
  // the light probe a user would pick in the file dialog (RenderingPipeline.cpp:229-243 -> ResourceManager::updateEnvironmentMap)
  if (!o.envFile.empty() && !pipeline->getResourceManager()->updateEnvironmentMap(o.envFile)) {
    std::fprintf(stderr, "bdpt_render: cannot load the environment map %s\n", o.envFile.c_str());
    return false;
  }
  Gui gui;  // what a user would have set in the GUI windows
  gui.overrides["Max Ray Depth"] = o.depth;
  gui.overrides["Material"] = o.mat;
  gui.overrides["Max frames to accumulate"] = o.accumLimit;
  if (o.denoise) gui.overrides["Ignore the denoise stage"] = 1;  // the check box's label while it is off (DenoisePass.cpp:139)
  if (o.denoiseRegression) gui.overrides["Skip Regression"] = 1;
  if (o.ao >= 0) gui.overrides["Num AO Rays"] = o.ao;
  if (o.ao >= 0 && o.aoRadiusSet) gui.overrides["AO radius"] = o.aoRadius;
  if (o.sky >= 0) gui.overrides["Num Sky Rays"] = o.sky;
  if (o.gi && o.giDirectOnly) gui.overrides["Shooting global illumination rays"] = 0;  // the check boxes' labels while they are on
  if (o.gi && o.giUniform) gui.overrides["Use cosine sampling"] = 0;                   // (SimpleDiffuseGIPass.cpp:82-84)
  pipeline->applyGui(&gui);
  if (!o.resume.empty() && !pipeline->loadCheckpoint(o.resume)) {  // continue an earlier run's frame sequence
    std::fprintf(stderr, "bdpt_render: cannot resume from %s (missing, or written for other passes / another frame size)\n", o.resume.c_str());
    return false;
  }
  return true;
}

// One pipeline on one GPU.  world == 0: the plain single-GPU run.  Otherwise rank `rank` of `world` (comm may be null
// for world == 1).
RankResult runRank(const Options& o, int device, const RankEnv& env) {
  RankResult res;
  const uint32_t rank = env.rank, world = env.world;
  const bool tiled = world > 0, writer = !tiled || rank == 0;
  std::unique_ptr<RenderingPipeline> pipeline(new RenderingPipeline());
  // a rank that has to leave a collective later (TileExchange::abort) releases its peers the same way a failed read-back does
  pipeline->setTilingAbortHandler([env] { env.failLate(); });
  const bool setUp = !env.injected("setup") && setUpRank(o, device, rank, world, env.comm, pipeline.get());
  // agreement point: a rank whose set-up failed (scene, tiling, a hipMalloc in initialize, the environment map, the
  // checkpoint) says so HERE, and every rank leaves — none enters a barrier or a collective its peer will never reach
  if (!env.agree(setUp)) {
    if (setUp) std::fprintf(stderr, "bdpt_render: rank %u leaves: the set-up of another rank failed\n", rank);
    return res;
  }

  if (o.tightRefit && (o.sway > 0.0f || o.bend > 0.0f) && !pipeline->setTightRefit()) {
    std::fprintf(stderr, "bdpt_render: setTightRefit failed\n");
    env.failLate();
    return res;
  }
  int warmup = o.warmup;
  if (warmup < 0 || warmup >= o.frames) warmup = 0;
  // --sway: a smooth displacement of every vertex before every frame (bdpt_update_geometry through the pipeline)
  std::vector<float> base, moved;
  float extent = 0.0f;
  if (o.sway > 0.0f && pipeline->getScene()) {
    base = pipeline->getScene()->positions;
    for (int a = 0; a < 3; a++) {
      float lo = 1e30f, hi = -1e30f;
      for (size_t i = a; i < base.size(); i += 3) {
        lo = std::min(lo, base[i]);
        hi = std::max(hi, base[i]);
      }
      extent = std::max(extent, hi - lo);
    }
  }
  // --bend: a procedural rig — kBendBones bones stacked along the scene's height, every vertex blended between the two
  // bones next to it — bent about the scene's foot before every frame (bdpt_set_skin once, then a bone palette per frame
  // through RenderingPipeline::updateSkinned; the vertices are skinned on the device)
  constexpr uint32_t kBendBones = 4;
  std::vector<float> bendBones, bendNormalBones;
  float bendPivot[3] = {0.0f, 0.0f, 0.0f};
  bool bendHasNormals = false;
  if (o.bend > 0.0f && pipeline->getScene()) {
    const Scene& sc = *pipeline->getScene();
    const size_t nv = sc.positions.size() / 3;
    float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
    for (size_t i = 0; i < nv * 3; i++) {
      lo[i % 3] = std::min(lo[i % 3], sc.positions[i]);
      hi[i % 3] = std::max(hi[i % 3], sc.positions[i]);
    }
    bendPivot[0] = 0.5f * (lo[0] + hi[0]);
    bendPivot[1] = lo[1];
    bendPivot[2] = 0.5f * (lo[2] + hi[2]);
    std::vector<float> weights(nv * 4, 0.0f);
    std::vector<uint16_t> ids(nv * 4, 0);
    const float height = std::max(hi[1] - lo[1], 1e-20f);
    for (size_t v = 0; v < nv; v++) {
      const float s = std::min(std::max((sc.positions[v * 3 + 1] - lo[1]) / height, 0.0f), 1.0f) * (float)(kBendBones - 1);
      const uint32_t k = std::min((uint32_t)s, kBendBones - 2);
      const float f = s - (float)k;
      ids[v * 4] = (uint16_t)k;
      ids[v * 4 + 1] = (uint16_t)(k + 1);
      weights[v * 4] = 1.0f - f;
      weights[v * 4 + 1] = f;
    }
    bendHasNormals = sc.normals.size() == nv * 3;
    bdpt_skin_desc sd{};
    sd.numVertices = (uint32_t)nv;
    sd.numBones = kBendBones;
    sd.positions = sc.positions.data();
    sd.normals = bendHasNormals ? sc.normals.data() : nullptr;
    sd.bitangents = sc.bitangents.size() == nv * 3 ? sc.bitangents.data() : nullptr;
    sd.boneWeights = weights.data();
    sd.boneIds = ids.data();
    if (!pipeline->setSkin(&sd)) {
      std::fprintf(stderr, "bdpt_render: setSkin failed\n");
      env.failLate();
      return res;
    }
    bendBones.assign(kBendBones * 16, 0.0f);
    bendNormalBones.assign(kBendBones * 16, 0.0f);
  }
  bool swayOk = true;
  auto frame = [&](int f) {
    if (!bendBones.empty()) {
      // bone k turns about the z axis through the pivot by k / (kBendBones - 1) of the frame's angle: p' = (p - c) R + c
      for (uint32_t k = 0; k < kBendBones; k++) {
        const float a = o.bend * std::sin(0.7f * (float)(f + 1)) * (float)k / (float)(kBendBones - 1);
        const float cs = std::cos(a), sn = std::sin(a);
        float* m = bendBones.data() + k * 16;
        const float R[9] = {cs, sn, 0.0f, -sn, cs, 0.0f, 0.0f, 0.0f, 1.0f};
        for (int r = 0; r < 3; r++)
          for (int c = 0; c < 3; c++) m[4 * r + c] = R[3 * r + c];
        for (int c = 0; c < 3; c++)
          m[12 + c] = bendPivot[c] - (bendPivot[0] * R[c] + bendPivot[1] * R[3 + c] + bendPivot[2] * R[6 + c]);
        m[15] = 1.0f;
        // (a rotation is its own inverse transpose; the translation plays no part in a normal)
        float* t = bendNormalBones.data() + k * 16;
        for (int r = 0; r < 3; r++)
          for (int c = 0; c < 3; c++) t[4 * r + c] = R[3 * r + c];
        t[15] = 1.0f;
      }
      swayOk = swayOk && pipeline->updateSkinned(bendBones.data(), bendHasNormals ? bendNormalBones.data() : nullptr, kBendBones);
    }
    if (!base.empty()) {
      moved = base;
      const float a = o.sway * extent * std::sin(0.7f * (float)(f + 1));
      for (size_t i = 0; i + 2 < moved.size(); i += 3) {
        moved[i] += a * std::sin(base[i + 1] * 6.0f / extent);
        moved[i + 2] += 0.5f * a * std::cos(base[i + 1] * 4.0f / extent);
      }
      swayOk = swayOk && pipeline->updateGeometry(moved.data());
    }
    pipeline->renderFrame();
  };
  for (int f = 0; f < warmup; f++) frame(f);
  (void)hipDeviceSynchronize();
  if (!env.barrier()) return res;
  auto t0 = std::chrono::steady_clock::now();
  for (int f = warmup; f < o.frames; f++) frame(f);
  if (!swayOk) {
    std::fprintf(stderr, "bdpt_render: updateGeometry / updateSkinned failed\n");
    env.failLate();
    return res;
  }
  (void)hipDeviceSynchronize();
  if (!env.barrier()) return res;  // the job is done when its slowest rank is
  res.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  // tiled: a collective — every rank calls it, every rank gets the frame
  std::vector<float> img = env.injected("readback") ? std::vector<float>() : pipeline->readOutput();
  if (img.size() != (size_t)o.W * o.H * 4) {
    std::fprintf(stderr, "bdpt_render: rank %u: reading the output back failed\n", rank);
    env.failLate();  // the peers may be inside the all-gather this rank never entered (or left early): release them
    return res;
  }
  if (writer) {
    double mean = 0;
    for (size_t i = 0; i < img.size(); i += 4) mean += img[i] + img[i + 1] + img[i + 2];
    if (o.direct)
      std::printf("%s %ux%u direct lighting%s: %d frames in %.2f ms (%.2f ms/frame), mean radiance %.6f", o.scene.c_str(), o.W, o.H,
                  o.directHints ? ", occluder hints" : "", o.frames - warmup, res.ms, res.ms / (o.frames - warmup),
                  mean / (3.0 * (double)(img.size() / 4)));
    else if (o.gi)
      std::printf("%s %ux%u diffuse GI (%s%s): %d frames in %.2f ms (%.2f ms/frame), mean radiance %.6f", o.scene.c_str(), o.W, o.H,
                  o.giDirectOnly ? "direct only" : "one bounce", o.giUniform ? ", uniform sampling" : ", cosine sampling", o.frames - warmup, res.ms,
                  res.ms / (o.frames - warmup), mean / (3.0 * (double)(img.size() / 4)));
    else if (o.restir())
      std::printf("%s %ux%u ReSTIR direct lighting%s%s, %d candidates, %d spatial neighbours within %d pixels%s: %d frames in %.2f ms (%.2f ms/frame), "
                  "mean radiance %.6f", o.scene.c_str(), o.W, o.H, o.risGgx ? " (GGX)" : "", o.areaLights ? ", emitter table" : "", o.ris, o.risSpatial,
                  o.risRadius, o.risTemporal ? ", temporal reuse" : "", o.frames - warmup, res.ms, res.ms / (o.frames - warmup),
                  mean / (3.0 * (double)(img.size() / 4)));
    else if (o.ris >= 0)
      std::printf("%s %ux%u resampled direct lighting%s%s%s, %d candidates, %d rays per pixel: %d frames in %.2f ms (%.2f ms/frame), mean radiance %.6f",
                  o.scene.c_str(), o.W, o.H, o.risGgx ? " (GGX)" : "", o.areaLights ? ", emitter table" : "", o.risHints ? ", occluder hints" : "",
                  o.ris, o.risSamples, o.frames - warmup, res.ms, res.ms / (o.frames - warmup), mean / (3.0 * (double)(img.size() / 4)));
    else if (o.sky >= 0)
      std::printf("%s %ux%u sky lighting%s, %d rays per pixel: %d frames in %.2f ms (%.2f ms/frame), mean radiance %.6f", o.scene.c_str(), o.W, o.H,
                  o.skyMis ? (o.skyGgx ? " (MIS, GGX; two rays a sample)" : " (MIS; two rays a sample)") : "", o.sky, o.frames - warmup, res.ms, res.ms / (o.frames - warmup), mean / (3.0 * (double)(img.size() / 4)));
    else if (o.ao >= 0)
      std::printf("%s %ux%u ambient occlusion, %d rays per pixel: %d frames in %.2f ms (%.2f ms/frame), mean ao %.6f", o.scene.c_str(), o.W, o.H,
                  o.ao, o.frames - warmup, res.ms, res.ms / (o.frames - warmup), mean / (3.0 * (double)(img.size() / 4)));
    else
      std::printf("%s %ux%u depth %d mat %d: %d frames in %.2f ms (%.2f ms/frame), mean radiance %.6f", o.scene.c_str(), o.W, o.H, o.depth, o.mat,
                  o.frames - warmup, res.ms, res.ms / (o.frames - warmup), mean / (3.0 * (double)(img.size() / 4)));
    if (tiled) std::printf(", %u GPU%s (interleaved stripes of %u rows, RCCL reduce-scatter + all-gather)", world, world == 1 ? "" : "s",
                           bdpt_stripe_rows(o.H, world));
    if (o.denoise && (o.sway > 0.0f || o.bend > 0.0f) && !o.noMotion && !tiled) std::printf(", denoiser history reprojected through the previous pose");
    if (o.tightRefit && (o.sway > 0.0f || o.bend > 0.0f)) std::printf(", references refitted by their pieces");
    std::printf("\n");
    writePfm(o.out.c_str(), img, o.W, o.H);
  }
  if (!o.checkpoint.empty() && !pipeline->saveCheckpoint(o.checkpoint)) {  // tiled: one file per rank (its rows)
    std::fprintf(stderr, "bdpt_render: cannot write %s\n", o.checkpoint.c_str());
    return res;
  }
  if (writer && !o.raw.empty()) {
    FILE* f = std::fopen(o.raw.c_str(), "wb");
    if (f) {
      std::fwrite(img.data(), 4, img.size(), f);
      std::fclose(f);
    }
  }
  res.rc = 0;
  return res;
}
}  // namespace

int main(int argc, char** argv) {
  Options o;
  for (int i = 1; i < argc; i++) {
    auto next = [&](const char* name) -> const char* {
      if (std::strcmp(argv[i], name) == 0 && i + 1 < argc) return argv[++i];
      return nullptr;
    };
    if (std::strcmp(argv[i], "--denoise") == 0) o.denoise = true;
    else if (std::strcmp(argv[i], "--denoise-regression") == 0) o.denoise = o.denoiseRegression = true;
    else if (std::strcmp(argv[i], "--area-lights") == 0) o.areaLights = true;
    else if (const char* v = next("--scene")) o.scene = v;
    else if (const char* v = next("--width")) o.W = (uint32_t)std::atoi(v);
    else if (const char* v = next("--height")) o.H = (uint32_t)std::atoi(v);
    else if (const char* v = next("--frames")) o.frames = std::atoi(v);
    else if (const char* v = next("--depth")) o.depth = std::atoi(v);
    else if (const char* v = next("--mat")) o.mat = std::atoi(v);
    else if (const char* v = next("--device")) o.device = std::atoi(v);
    else if (const char* v = next("--accum-limit")) o.accumLimit = std::atoi(v);
    else if (const char* v = next("--out")) o.out = v;
    else if (const char* v = next("--raw")) o.raw = v;
    else if (const char* v = next("--checkpoint")) o.checkpoint = v;
    else if (const char* v = next("--resume")) o.resume = v;
    else if (const char* v = next("--env")) o.envFile = v;
    else if (const char* v = next("--inflight")) o.inflight = std::atoi(v);
    else if (const char* v = next("--warmup")) o.warmup = std::atoi(v);  // of --frames: rendered before the clock starts (first-use allocations)
    else if (const char* v = next("--sway")) o.sway = (float)std::atof(v);
    else if (const char* v = next("--bend")) o.bend = (float)std::atof(v);
    else if (const char* v = next("--ao")) o.ao = std::max(0, std::atoi(v));
    else if (const char* v = next("--ao-radius")) o.aoRadius = (float)std::atof(v), o.aoRadiusSet = true;
    else if (const char* v = next("--sky")) o.sky = std::max(0, std::atoi(v));
    else if (const char* v = next("--sky-clamp")) o.skyClamp = (float)std::atof(v), o.skyClampSet = true;
    else if (std::strcmp(argv[i], "--sky-mis") == 0) o.skyMis = true;
    else if (std::strcmp(argv[i], "--sky-ggx") == 0) o.skyGgx = true;
    else if (std::strcmp(argv[i], "--gi") == 0) o.gi = true;
    else if (std::strcmp(argv[i], "--gi-direct-only") == 0) o.giDirectOnly = true;
    else if (std::strcmp(argv[i], "--gi-uniform") == 0) o.giUniform = true;
    else if (const char* v = next("--ris")) o.ris = std::max(0, std::atoi(v));
    else if (const char* v = next("--ris-samples")) o.risSamples = std::atoi(v), o.risSamplesSet = true;
    else if (const char* v = next("--ris-clamp")) o.risClamp = (float)std::atof(v), o.risClampSet = true;
    else if (std::strcmp(argv[i], "--ris-ggx") == 0) o.risGgx = true;
    else if (std::strcmp(argv[i], "--ris-hints") == 0) o.risHints = true;
    else if (const char* v = next("--ris-spatial")) o.risSpatial = std::atoi(v);
    else if (const char* v = next("--ris-radius")) o.risRadius = std::atoi(v), o.risRadiusSet = true;
    else if (const char* v = next("--ris-max-m")) o.risMaxM = std::atoi(v), o.risMaxMSet = true;
    else if (std::strcmp(argv[i], "--ris-temporal") == 0) o.risTemporal = true;
    else if (std::strcmp(argv[i], "--direct") == 0) o.direct = true;
    else if (std::strcmp(argv[i], "--direct-hints") == 0) o.directHints = true;
    else if (std::strcmp(argv[i], "--no-motion") == 0) o.noMotion = true;
    else if (std::strcmp(argv[i], "--tight-refit") == 0) o.tightRefit = true;
    else if (const char* v = next("--gpus")) o.gpus = std::atoi(v);
    else if (const char* v = next("--rank")) o.rank = std::atoi(v);
    else if (const char* v = next("--world")) o.world = std::atoi(v);
    else if (const char* v = next("--id-file")) o.idFile = v;
    else if (const char* v = next("--job-id")) o.jobId = v;  // names THIS run of the job: the id file of another run is not accepted
    else {
      std::fprintf(stderr, "usage: bdpt_render [--scene cornell|atrium|FILE.fscene|FILE.obj] [--width W] [--height H] [--frames N] [--depth D] "
                           "[--mat 0|1] [--accum-limit N] [--denoise | --denoise-regression] [--area-lights] [--out file.pfm] [--raw file.f32] "
                           "[--resume file.ckpt] [--checkpoint file.ckpt] [--env probe.hdr|image|Black] [--inflight N] [--warmup N] [--sway A] [--bend A] [--no-motion] [--tight-refit] [--ao N [--ao-radius R]] [--gi [--gi-direct-only] [--gi-uniform]] [--direct [--direct-hints]] [--sky N [--sky-clamp C] [--sky-mis [--sky-ggx]]] [--ris M [--ris-samples K] [--ris-ggx] [--ris-hints] [--ris-clamp C] [--ris-spatial N [--ris-radius R]] [--ris-temporal] [--ris-max-m C]] "
                           "[--gpus N | --rank R --world N --id-file F [--job-id J] [--device D]]\n");
      return 2;
    }
  }
  if (o.ao >= 0 && (o.ao < 1 || o.ao > (int)BDPT_AO_MAX_SAMPLES || o.gpus > 0 || o.world > 0 || (o.aoRadiusSet && !(o.aoRadius > 0.0f)))) {
    std::fprintf(stderr, "bdpt_render: --ao N needs N in 1 .. %u rays per pixel, --ao-radius R > 0 when given, and one GPU (no --gpus / --world)\n",
                 BDPT_AO_MAX_SAMPLES);
    return 2;
  }
  // --ao replaces the BDPT, accumulation and denoise passes: the switches only they read are refused, not ignored
  if (o.ao >= 0 && (o.denoise || o.areaLights || o.noMotion)) {
    std::fprintf(stderr, "bdpt_render: --ao N renders the G-buffer and the ambient occlusion pass only: not with --denoise, --denoise-regression, "
                         "--area-lights or --no-motion\n");
    return 2;
  }
  if (o.ao < 0 && o.aoRadiusSet) {
    std::fprintf(stderr, "bdpt_render: --ao-radius R goes with --ao N\n");
    return 2;
  }
  if (o.gi && (o.ao >= 0 || o.gpus > 0 || o.world > 0)) {
    std::fprintf(stderr, "bdpt_render: --gi renders on one GPU (no --gpus / --world) and not together with --ao N\n");
    return 2;
  }
  // --gi replaces the BDPT and denoise passes: the switches only they read are refused, not ignored
  if (o.gi && (o.denoise || o.areaLights || o.noMotion)) {
    std::fprintf(stderr, "bdpt_render: --gi renders the G-buffer, the diffuse GI pass and the accumulation pass only: not with --denoise, "
                         "--denoise-regression, --area-lights or --no-motion\n");
    return 2;
  }
  if (!o.gi && (o.giDirectOnly || o.giUniform)) {
    std::fprintf(stderr, "bdpt_render: --gi-direct-only and --gi-uniform go with --gi\n");
    return 2;
  }
  if (o.direct && (o.ao >= 0 || o.gi || o.gpus > 0 || o.world > 0)) {
    std::fprintf(stderr, "bdpt_render: --direct renders on one GPU (no --gpus / --world) and not together with --ao N or --gi\n");
    return 2;
  }
  // --direct replaces the BDPT, accumulation and denoise passes: the switches only they read are refused, not ignored
  if (o.direct && (o.denoise || o.areaLights || o.noMotion)) {
    std::fprintf(stderr, "bdpt_render: --direct renders the G-buffer and the direct lighting pass only: not with --denoise, "
                         "--denoise-regression, --area-lights or --no-motion\n");
    return 2;
  }
  if (!o.direct && o.directHints) {
    std::fprintf(stderr, "bdpt_render: --direct-hints goes with --direct\n");
    return 2;
  }
  if (o.sky >= 0 && (o.sky < 1 || o.sky > (int)BDPT_SKY_MAX_SAMPLES || o.gpus > 0 || o.world > 0 || (o.skyClampSet && !(o.skyClamp > 0.0f)))) {
    std::fprintf(stderr, "bdpt_render: --sky N needs N in 1 .. %u rays per pixel, --sky-clamp C > 0 when given, and one GPU (no --gpus / --world)\n",
                 BDPT_SKY_MAX_SAMPLES);
    return 2;
  }
  if (o.sky >= 0 && (o.envFile.empty() || o.envFile == "Black")) {
    std::fprintf(stderr, "bdpt_render: --sky N samples an environment map: it needs --env FILE\n");
    return 2;
  }
  // --sky replaces the BDPT and denoise passes: the switches only they read are refused, not ignored
  if (o.sky >= 0 && (o.ao >= 0 || o.gi || o.direct || o.denoise || o.areaLights || o.noMotion)) {
    std::fprintf(stderr, "bdpt_render: --sky N renders the G-buffer, the sky lighting pass and the accumulation pass only: not with --ao N, --gi, "
                         "--direct, --denoise, --denoise-regression, --area-lights or --no-motion\n");
    return 2;
  }
  if (o.sky < 0 && o.skyClampSet) {
    std::fprintf(stderr, "bdpt_render: --sky-clamp C goes with --sky N\n");
    return 2;
  }
  if ((o.skyMis && o.sky < 0) || (o.skyGgx && !o.skyMis)) {
    std::fprintf(stderr, "bdpt_render: --sky-mis goes with --sky N, and --sky-ggx with --sky-mis\n");
    return 2;
  }
  if (o.ris < 0 && (o.risSamplesSet || o.risGgx || o.risHints || o.risClampSet)) {
    std::fprintf(stderr, "bdpt_render: --ris-samples K, --ris-ggx, --ris-hints and --ris-clamp C go with --ris M\n");
    return 2;
  }
  if (o.ris >= 0 && (o.ris < 1 || o.ris > (int)BDPT_RIS_MAX_CANDIDATES || o.risSamples < 1 || o.risSamples > (int)BDPT_RIS_MAX_SAMPLES ||
                     o.gpus > 0 || o.world > 0 || (o.risClampSet && !(o.risClamp > 0.0f)))) {
    std::fprintf(stderr, "bdpt_render: --ris M needs M in 1 .. %u candidates, --ris-samples K in 1 .. %u, --ris-clamp C > 0 when given, and one GPU "
                         "(no --gpus / --world)\n", BDPT_RIS_MAX_CANDIDATES, BDPT_RIS_MAX_SAMPLES);
    return 2;
  }
  if (o.ris < 0 && (o.risSpatial != 0 || o.risRadiusSet || o.risTemporal || o.risMaxMSet)) {
    std::fprintf(stderr, "bdpt_render: --ris-spatial N, --ris-radius R, --ris-temporal and --ris-max-m C go with --ris M\n");
    return 2;
  }
  if (o.ris >= 0 && (o.risSpatial < 0 || o.risSpatial > (int)BDPT_REUSE_MAX_NEIGHBORS || (o.risRadiusSet && o.risSpatial <= 0) || o.risRadius < 1 ||
                     o.risRadius > (int)BDPT_REUSE_MAX_RADIUS || (o.risMaxMSet && (!o.restir() || o.risMaxM < 1)) ||
                     (o.restir() && (o.risSamples != 1 || o.risHints || o.inflight > 1 || o.sway > 0.0f || o.bend > 0.0f)))) {
    std::fprintf(stderr, "bdpt_render: --ris-spatial N needs N in 0 .. %u, --ris-radius R in 1 .. %u with --ris-spatial, --ris-max-m C >= 1 with "
                         "--ris-spatial or --ris-temporal; reservoir reuse takes one sample, no hints, one frame in flight and a scene that does not "
                         "move (no --ris-samples, --ris-hints, --inflight, --sway, --bend)\n", BDPT_REUSE_MAX_NEIGHBORS, BDPT_REUSE_MAX_RADIUS);
    return 2;
  }
  // --ris replaces the BDPT and denoise passes: the switches only they read are refused, not ignored (--area-lights is read)
  if (o.ris >= 0 && (o.ao >= 0 || o.gi || o.direct || o.sky >= 0 || o.denoise || o.noMotion)) {
    std::fprintf(stderr, "bdpt_render: --ris M renders the G-buffer, the resampled direct lighting pass and the accumulation pass only: not with "
                         "--ao N, --gi, --direct, --sky N, --denoise, --denoise-regression or --no-motion\n");
    return 2;
  }
  if (o.gpus < 0 || o.gpus > 64 || (o.gpus > 0 && o.world > 0)) {
    std::fprintf(stderr, "bdpt_render: --gpus N (ranks as threads) or --rank R --world N --id-file F (one process per rank), not both\n");
    return 2;
  }

  if (o.world > 0) {  // one process per GPU: this is rank --rank of --world
    if (o.rank < 0 || o.rank >= o.world || o.idFile.empty()) {
      std::fprintf(stderr, "bdpt_render: --world N needs --rank R in [0, N) and --id-file F\n");
      return 2;
    }
    if (hipSetDevice(o.device) != hipSuccess) {
      std::fprintf(stderr, "bdpt_render: no HIP device %d\n", o.device);
      return 1;
    }
    ncclUniqueId id;
    ncclComm_t comm = nullptr;
    if (!bdpt::exchangeUniqueIdThroughFile(o.idFile, (uint32_t)o.rank, &id, 120.0, bdpt::jobNonce(o.jobId)) ||
        ncclCommInitRank(&comm, o.world, id, o.rank) != ncclSuccess) {
      std::fprintf(stderr, "bdpt_render: rank %d could not join the communicator through %s\n", o.rank, o.idFile.c_str());
      return 1;
    }
    if (o.rank == 0) bdpt::retireUniqueIdFile(o.idFile);  // every rank has joined: the file has served (single use)
    RankEnv env;
    env.comm = comm;
    env.rank = (uint32_t)o.rank;
    env.world = (uint32_t)o.world;
    RankResult r = runRank(o, o.device, env);
    if (r.rc == 0) ncclCommDestroy(comm);  // (after a failure the communicator was aborted, or peers may be gone: no orderly teardown)
    return r.rc;
  }

  if (o.gpus > 0) {  // N ranks as threads of this process, GPUs device .. device + N - 1
    int have = 0;
    if (hipGetDeviceCount(&have) != hipSuccess || have < o.device + o.gpus) {
      std::fprintf(stderr, "bdpt_render: --gpus %d from device %d, but %d HIP device(s) are visible\n", o.gpus, o.device, have);
      return 1;
    }
    std::vector<int> devs((size_t)o.gpus);
    for (int i = 0; i < o.gpus; i++) devs[(size_t)i] = o.device + i;
    std::vector<ncclComm_t> comms((size_t)o.gpus, nullptr);
    const ncclResult_t nr = ncclCommInitAll(comms.data(), o.gpus, devs.data());
    if (nr != ncclSuccess) {
      std::fprintf(stderr, "bdpt_render: ncclCommInitAll: %s\n", ncclGetErrorString(nr));
      return 1;
    }
    bdpt::RankGroup group(o.gpus);
    std::vector<RankResult> results((size_t)o.gpus);
    std::vector<std::thread> threads;
    auto envOf = [&](int r) {
      RankEnv env;
      env.group = &group;
      env.comm = comms[(size_t)r];
      env.rank = (uint32_t)r;
      env.world = (uint32_t)o.gpus;
      return env;
    };
    // the watcher: once a rank has called abort(), every communicator is aborted so that no peer stays inside a collective
    std::atomic<bool> ranksDone{false}, commsAborted{false};
    std::thread watcher([&] {
      while (!ranksDone.load()) {
        if (group.aborted()) {
          for (ncclComm_t c : comms) ncclCommAbort(c);
          commsAborted.store(true);
          return;
        }
        std::this_thread::sleep_for(std::chrono::milliseconds(20));
      }
    });
    for (int r = 1; r < o.gpus; r++) threads.emplace_back([&, r] { results[(size_t)r] = runRank(o, devs[(size_t)r], envOf(r)); });
    results[0] = runRank(o, devs[0], envOf(0));
    for (std::thread& t : threads) t.join();
    ranksDone.store(true);
    watcher.join();
    int rc = 0;
    for (int r = 0; r < o.gpus; r++) {
      if (results[(size_t)r].rc != 0) rc = 1;
      if (!commsAborted.load()) ncclCommDestroy(comms[(size_t)r]);
    }
    return rc;
  }

  return runRank(o, o.device, RankEnv{}).rc;
}
