// api_frame.cpp — the frame of the C ABI (include/bdpt.h): bdpt_resize / bdpt_resize_stripes and the tile they describe,
// the G-buffer passes, the BDPT frame pipeline behind the bdpt_execute* family, adaptive sampling, bdpt_prepare, the
// splat buffer, resolve / accumulate and tile pack / unpack.  Workspaces are sized by bdpt_resize and bdpt_prepare (both
// allocate and synchronise: not inside a capture), so the passes neither allocate nor synchronise and can be captured
// into a hipGraph.  The one exception is spelled out in bdpt.h: bdpt_execute(in = NULL), the light-group frames and a
// frame with BDPT_PARAM_AREA_LIGHTS allocate their optional buffers on first use when bdpt_prepare was not called, and
// refuse (BDPT_E_STATE) to do so while the stream is being captured.
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "api_common.hpp"

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

// What bdpt_resize and bdpt_resize_stripes share: the checks (a refused call leaves the old frame in place), the drop, then
// every workspace of a `width` x `height` frame of which this context renders `tile`.
int resizeRows(bdpt_ctx* c, TileDesc tile, uint32_t width, uint32_t height, uint32_t maxDepth) {
  if (maxDepth > BDPT_MAX_DEPTH) return refuse(c, BDPT_E_LIMIT, "resize", "maxDepth exceeds BDPT_MAX_DEPTH");
  if ((uint64_t)width * height >= (1ull << 32) || (uint64_t)tile.sl.owners * tile.sl.chunkRows * width >= (1ull << 32)) {
    fail(c, "resize: frame too large");
    return BDPT_E_LIMIT;
  }
  if ((uint64_t)tile.rows * width >= (1ull << 24)) {
    fail(c, "resize: a tile holds at most 2^24 - 1 pixels (path ids pack the pixel in 24 bits); render in smaller tiles");
    return BDPT_E_LIMIT;
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  dropFrame(c);
  c->frame.tile = std::move(tile);
  c->frame.W = width;
  c->frame.H = height;
  c->frame.maxDepth = maxDepth;
  PathBuf P{};
  P.Np = c->frame.tile.rows * width;
  P.D1 = std::max<uint32_t>(maxDepth, 1) + 1;
  const size_t np = std::max<uint32_t>(P.Np, 1);
  int rc;
  {
    std::vector<uint32_t> pix;
    pix.reserve(np);
    for (const auto& rr : c->frame.tile.rowRanges)
      for (uint32_t y = rr.first; y < rr.second; y++)
        for (uint32_t x = 0; x < width; x++) pix.push_back(y * width + x);
    if ((rc = devUpload(c, c->frame.allocs, &P.pix, pix.data(), pix.size()))) return rc;
  }
  if ((rc = devAlloc(c, c->frame.allocs, &P.v, (size_t)2 * P.D1 * NF4 * 4 * np))) return rc;
  if ((rc = devAlloc(c, c->frame.allocs, &P.rayDir, (size_t)6 * np))) return rc;
  if ((rc = devAlloc(c, c->frame.allocs, &P.seedL, np))) return rc;
  if ((rc = devAlloc(c, c->frame.allocs, &P.eyeLast, np))) return rc;
  if ((rc = devAlloc(c, c->frame.allocs, &P.lightLast, np))) return rc;
  if ((rc = devAlloc(c, c->frame.allocs, &P.lightReal, np))) return rc;
  // a path queue = kNumSubQueues lists; workgroup b appends to list b % kNumSubQueues
  // (+ one workgroup's worth of slack)
  P.pathSubCap = (uint32_t)((((uint64_t)wavesFor(np) + kNumSubQueues - 1) / kNumSubQueues + 1) * kWave);
  const size_t qcap = (size_t)P.pathSubCap * kNumSubQueues;
  for (int q = 0; q < 3; q++)
    if ((rc = devAlloc(c, c->frame.allocs, &P.queue[q], qcap))) return rc;
  if ((rc = devAlloc(c, c->frame.allocs, &P.qcount, (size_t)kCursorWords))) return rc;
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
    if (cap >= (1ull << 32) - 1) return refuse(c, BDPT_E_LIMIT, "resize", "shadow-ray queue would exceed 2^32 entries; render in smaller tiles");
    P.raySubCap[RAY_TERMS] = (uint32_t)subCapTerms;
    P.raySubCap[RAY_PAIRS] = (uint32_t)subCapPairs;
    P.rayBase[RAY_TERMS] = 0;
    P.rayBase[RAY_PAIRS] = (uint32_t)(subCapTerms * kNumRaySubQueues);
    P.rayCap = (uint32_t)cap;
    if ((rc = devAlloc(c, c->frame.allocs, &P.rayQ, (size_t)7 * cap))) return rc;
    if ((rc = devAlloc(c, c->frame.allocs, &P.rayContrib, (size_t)3 * cap))) return rc;
    if ((rc = devAlloc(c, c->frame.allocs, &P.rayVis, (size_t)cap))) return rc;
    if ((rc = devAlloc(c, c->frame.allocs, &P.slotRay, (size_t)slots * np))) return rc;
    if ((rc = devAlloc(c, c->frame.allocs, &P.splatPix, (size_t)D * np))) return rc;
    // Lazy rounds: each costs three small launches, so small tiles (multi-GPU bands) take fewer, larger ones.
    // Lazy rounds: each costs three small launches and cannot finish faster than its slowest ray, so there are few:
    // two or three rounds of kLazyBatchDiv-th shares, the last of which takes every candidate that is left.
    c->frame.lazyRounds = np >= (1u << 18) ? 3 : 2;
    if (const char* e = std::getenv("BDPT_LAZY_ROUNDS")) {  // measurement knob (tools/prof_tile.sh): 1 .. kMaxLazyRounds
      const int v = std::atoi(e);
      if (v >= 1 && v <= kMaxLazyRounds) c->frame.lazyRounds = v;
    }
    // the largest batch any round can ask for: the last round of the front-loaded schedule takes what is left
    const uint32_t batch = numConnectPairs(D);
    if ((rc = devAlloc(c, c->frame.allocs, &P.misE, (size_t)(D + 1) * np))) return rc;
    if ((rc = devAlloc(c, c->frame.allocs, &P.misL, (size_t)(D + 1) * np))) return rc;
    if ((rc = devAlloc(c, c->frame.allocs, &P.lazyCursor, np))) return rc;
    if ((rc = devAlloc(c, c->frame.allocs, &P.lazyRay, (size_t)std::max<uint32_t>(batch, 1) * np))) return rc;
  }
  if (std::getenv("BDPT_NO_HINTS") == nullptr) {
    if ((rc = devAlloc(c, c->frame.allocs, &c->frame.hintPix, (size_t)width * height))) return rc;
    HIPCHK(c, hipMemset(c->frame.hintPix, 0xFF, (size_t)width * height * sizeof(uint32_t)));
  }
  const size_t splatU64 = (size_t)c->frame.tile.sl.owners * c->frame.tile.sl.chunkRows * width * 4;
  if ((rc = devAlloc(c, c->frame.allocs, &c->frame.ownSplat, splatU64))) return rc;
  c->frame.splat = c->frame.ownSplat;
  if ((rc = devAlloc(c, c->frame.allocs, &c->frame.counters, 1))) return rc;
  HIPCHK(c, hipMemset(c->frame.splat, 0, splatU64 * sizeof(unsigned long long)));
  HIPCHK(c, hipMemset(c->frame.counters, 0, sizeof(DevCounters)));
  c->frame.P = P;
  if (!c->evCreated) {
    for (int i = 0; i <= kMaxStages; i++) HIPCHK(c, hipEventCreate(&c->ev[i]));
    for (hipEvent_t& e : c->sideEv) HIPCHK(c, hipEventCreate(&e));
    c->evCreated = true;
  }
  c->frame.have = true;
  return BDPT_OK;
}

// the six channels of the built-in primary stage; all or nothing
int allocOwnGbuffer(bdpt_ctx* c) {
  if (c->frame.ownGb.worldPosition) return BDPT_OK;
  const size_t n = (size_t)c->frame.W * c->frame.H;
  DevPool pool;
  bdpt_gbuffer g{};
  int rc;
  if ((rc = devAlloc(c, pool, &g.worldPosition, n * 4)) || (rc = devAlloc(c, pool, &g.worldNormal, n * 4)) ||
      (rc = devAlloc(c, pool, &g.materialDiffuse, n * 4)) || (rc = devAlloc(c, pool, &g.materialSpecRough, n * 4)) ||
      (rc = devAlloc(c, pool, &g.materialExtraParams, n * 4)) || (rc = devAlloc(c, pool, &g.emissive, n * 4)))
    return rc;
  pool.moveTo(c->frame.allocs);
  c->frame.ownGb = g;
  return BDPT_OK;
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

}  // namespace

extern "C" {

int bdpt_resize(bdpt_ctx* c, uint32_t width, uint32_t height, bdpt_tile tile, uint32_t maxDepth) {
  if (!c) return BDPT_E_INVALID;
  if (!width || !height || tile.y0 > tile.y1 || tile.y1 > height) return refuse(c, BDPT_E_INVALID, "resize", "bad frame or tile");
  TileDesc t;  // (stripes: the default, a contiguous band)
  if (tile.y1 > tile.y0) t.rowRanges.push_back({tile.y0, tile.y1});
  t.rows = tile.y1 - tile.y0;
  t.sl = SplatLayout{1, 1, height};  // frame order
  return resizeRows(c, std::move(t), width, height, maxDepth);
}

// Interleaved stripes: rows are dealt to `numOwners` contexts in stripes of `stripeRows`; this one
// renders the stripes s with s % numOwners == owner.  The splat buffer becomes owner-major (bdpt_get_tile_info).
int bdpt_resize_stripes(bdpt_ctx* c, uint32_t width, uint32_t height, bdpt_stripes st, uint32_t maxDepth) {
  if (!c) return BDPT_E_INVALID;
  if (!width || !height || !st.stripeRows || !st.numOwners || st.owner >= st.numOwners) {
    fail(c, "resize_stripes: bad frame or stripe description");
    return BDPT_E_INVALID;
  }
  TileDesc t;
  const uint32_t numStripes = (height + st.stripeRows - 1) / st.stripeRows;
  for (uint32_t s = st.owner; s < numStripes; s += st.numOwners) {
    const uint32_t a = s * st.stripeRows, b = std::min(height, a + st.stripeRows);
    t.rowRanges.push_back({a, b});
    t.rows += b - a;
  }
  t.stripes = st;
  t.sl = SplatLayout{st.stripeRows, st.numOwners, ((numStripes + st.numOwners - 1) / st.numOwners) * st.stripeRows};
  return resizeRows(c, std::move(t), width, height, maxDepth);
}

uint32_t bdpt_stripe_rows(uint32_t height, uint32_t numOwners) {
  const uint32_t per = height / std::max(1u, numOwners * 4u);
  return std::max(1u, std::min(8u, per));
}
int bdpt_get_tile_info(const bdpt_ctx* c, bdpt_tile_info* out) {
  if (!c || !out) return BDPT_E_INVALID;
  if (!c->frame.have) return BDPT_E_STATE;
  out->numRows = c->frame.tile.rows;
  out->numPixels = c->frame.P.Np;
  out->chunkRows = c->frame.tile.sl.chunkRows;
  out->numRowRanges = (uint32_t)c->frame.tile.rowRanges.size();
  out->splatU64 = (uint64_t)c->frame.tile.sl.owners * c->frame.tile.sl.chunkRows * c->frame.W * 4;
  out->chunkU64 = (uint64_t)c->frame.tile.sl.chunkRows * c->frame.W * 4;
  return BDPT_OK;
}

int bdpt_tile_row_ranges(const bdpt_ctx* c, uint32_t* out_first_last, uint32_t cap) {
  if (!c || !out_first_last) return BDPT_E_INVALID;
  if (!c->frame.have) return BDPT_E_STATE;
  const uint32_t n = std::min<uint32_t>(cap, (uint32_t)c->frame.tile.rowRanges.size());
  for (uint32_t i = 0; i < n; i++) {
    out_first_last[2 * i] = c->frame.tile.rowRanges[i].first;
    out_first_last[2 * i + 1] = c->frame.tile.rowRanges[i].second;
  }
  return (int)n;
}

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
  G.W = c->frame.W;
  G.H = c->frame.H;
  G.Np = c->frame.P.Np;
  G.pix = c->frame.P.pix;
  G.gb = *out;
  G.counters = nullptr;  // primary rays are tallied analytically by bdpt_get_counters (one per tile pixel)
  G.hintPix = c->frame.hintPix;
  if (c->frame.hintPix && c->frame.tile.rows != c->frame.H && (!c->frame.hintCamValid || std::memcmp(&c->frame.hintCam, &c->cam, sizeof(bdpt_camera)) != 0)) {
    GBufferDev A = G;
    A.Np = c->frame.W * c->frame.H;
    A.pix = nullptr;
    launchHintFill(c->scene.S, A, st);
    c->frame.hintCam = c->cam;
    c->frame.hintCamValid = true;
  }
  if (prevPosition) {
    MotionDev M{};
    M.prevPose = c->scene.prevPose;
    M.prevPosition = reinterpret_cast<float4*>(prevPosition);
    launchGBufferMotion(c->scene.S, G, M, st);
  } else {
    launchGBuffer(c->scene.S, G, st);
  }
  HIPCHK(c, hipGetLastError());
  c->lastStream = st;
  return BDPT_OK;
}
}  // namespace

int bdpt_gbuffer_execute(bdpt_ctx* c, const bdpt_gbuffer_params* gp, const bdpt_gbuffer* out, void* stream) {
  if (!c || !gp || !out) return BDPT_E_INVALID;
  if (!c->scene.have || !c->haveCamera || !c->frame.have) {
    fail(c, "gbuffer_execute: scene, camera and size must be set first");
    return BDPT_E_STATE;
  }
  return gbufferRun(c, gp, out, nullptr, stream);
}

int bdpt_gbuffer_execute_motion(bdpt_ctx* c, const bdpt_gbuffer_params* gp, const bdpt_gbuffer* out, float* prevPosition, void* stream) {
  if (!c || !gp || !out) return BDPT_E_INVALID;
  if (!c->scene.have || !c->haveCamera || !c->frame.have) {
    fail(c, "gbuffer_execute_motion: scene, camera and size must be set first");
    return BDPT_E_STATE;
  }
  if (!c->scene.prevPose) return refuse(c, BDPT_E_STATE, "gbuffer_execute_motion", "no previous pose (bdpt_prepare(BDPT_PREPARE_MOTION) first)");
  if (!aligned(prevPosition, 16)) return refuse(c, BDPT_E_INVALID, "gbuffer_execute_motion", "prevPosition missing or not 16-byte aligned");
  return gbufferRun(c, gp, out, prevPosition, stream);
}

namespace {
// argument checks shared by bdpt_execute and bdpt_execute_tail, and the per-frame constants the kernels take
int frameSetup(bdpt_ctx* c, const bdpt_params* p, const bdpt_gbuffer* in, float* out, hipStream_t st, FrameDev& F) {
  if (!c || !p || !out) return BDPT_E_INVALID;
  ENTER(c);
  if (!in) {  // the context's own channels: the primary stage runs inside bdpt_execute
    if (!c->frame.have) return refuse(c, BDPT_E_STATE, "execute", "scene, camera and size must be set first");
    if (!c->frame.ownGb.worldPosition) {  // bdpt_prepare(BDPT_PREPARE_PRIMARY) was not called: allocate now, unless capturing
      if (streamIsCapturing(st)) {
        fail(c, "execute: the built-in primary stage needs bdpt_prepare(BDPT_PREPARE_PRIMARY) before stream capture");
        return BDPT_E_STATE;
      }
      if (int rc = allocOwnGbuffer(c)) return rc;
    }
    in = &c->frame.ownGb;
  }
  if (!c->scene.have || !c->haveCamera || !c->frame.have) return refuse(c, BDPT_E_STATE, "execute", "scene, camera and size must be set first");
  if (p->maxDepth > c->frame.maxDepth) return refuse(c, BDPT_E_LIMIT, "execute", "params.maxDepth exceeds the depth given to bdpt_resize");
  if (p->matIndex > 1) return refuse(c, BDPT_E_INVALID, "execute", "matIndex must be 0 (GGX) or 1 (Lambertian)");
  // clampVec(x, hi) returns hi itself for a NaN or negative hi, and a light-tracing term c in [0, hi] lands as
  // (uint64_t)(c * 2^32) (toFixed, device_math.hpp), a conversion that is defined only below 2^64 (include/bdpt.h, bdpt_params)
  if (!(p->clampUpper >= 0.0f)) return refuse(c, BDPT_E_INVALID, "execute", "clampUpper must be a number >= 0");
  if (!(p->flags & BDPT_PARAM_NO_SPLAT) && p->clampUpper > BDPT_MAX_CLAMP_UPPER_SPLAT)
    return refuse(c, BDPT_E_LIMIT, "execute", "clampUpper exceeds BDPT_MAX_CLAMP_UPPER_SPLAT in a frame with light-tracing splats");
  if (!in->worldPosition || !in->worldNormal || !in->materialDiffuse || !in->materialSpecRough || !in->emissive) {
    fail(c, "execute: G-buffer channels missing");
    return BDPT_E_INVALID;
  }
  F = FrameDev{};
  F.cam = c->cam;
  F.p = *p;
  F.W = c->frame.W;
  F.H = c->frame.H;
  F.sl = c->frame.tile.sl;
  F.out = out;
  F.splat = c->frame.splat;
  F.gb = *in;
  F.counters = c->frame.counters;  // ray tallies are always on; node/triangle visits need BDPT_PARAM_COUNTERS
  F.envMap = c->env.envMap;
  F.envW = c->env.width;
  F.envH = c->env.height;
  for (int k = 0; k < 3; k++) F.envColor[k] = c->env.color[k];
  F.hintPix = c->frame.hintPix;
  return BDPT_OK;
}

// Connection pairs whose contribution is exactly zero, for the pixels no visible connection has saturated
// yet (DESIGN.md "Lazy connection rounds"), then the splat fold-in unless the caller defers it.
// V: the frame's variant (FrameVariant), for the lazy check and the resolve.
int connectionTail(bdpt_ctx* c, const FrameDev& F, hipStream_t st, const FrameVariant& V) {
  const PathBuf& P = c->frame.P;
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
    for (int r = 0; r < c->frame.lazyRounds && left > 0; r++) {
      const int batch = (r + 1 == c->frame.lazyRounds) ? left : (b0 < left ? b0 : left);
      left -= batch;
      uint32_t* list = P.queue[1 + (r & 1)];
      uint32_t* next = P.queue[1 + ((r + 1) & 1)];
      HIPCHK(c, hipMemsetAsync(P.rayCount + (size_t)RAY_PAIRS * kRayCursorBlock, 0, kRayCursorBlock * sizeof(uint32_t), st));
      HIPCHK(c, hipMemsetAsync(P.rayHead + (size_t)RAY_PAIRS * kRayCursorBlock, 0, kRayCursorBlock * sizeof(uint32_t), st));
      launchLazyGen(F, P, list, P.lazyCount + (size_t)r * kCursorBlock, batch, st);
      stageMark(c, st, "lazy_gen");
      launchTraceShadow(c->scene.S, F, P, RAY_PAIRS, c->grids, c->numCUs, st);
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
    V.area = c->scene.area;  // n == 0 (no emitter): the plain instances
    if (V.kind == FrameKind::Groups && V.area.n) V.groups.areaW = V.area.total;
  }
  const PathBuf& P = c->frame.P;
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
    if (int rc = bdpt_gbuffer_execute(c, &gp, &c->frame.ownGb, stream)) return rc;
  }

  c->numStages = 0;
  c->numSideStages = 0;
  if (c->timing) HIPCHK(c, hipEventRecord(c->ev[0], st));
  HIPCHK(c, hipMemsetAsync(P.qcount, 0, (size_t)kCursorWords * sizeof(uint32_t), st));
  HIPCHK(c, hipMemsetAsync(c->frame.splat, 0, (size_t)c->frame.tile.sl.owners * c->frame.tile.sl.chunkRows * c->frame.W * 4 * sizeof(unsigned long long), st));
  if (V.kind == FrameKind::Groups)
    HIPCHK(c, hipMemsetAsync(V.groups.splat, 0, (size_t)V.groups.numGroups * V.groups.framePix * 4 * sizeof(unsigned long long), st));
  if (!(p->flags & BDPT_PARAM_KEEP_COUNTERS)) HIPCHK(c, hipMemsetAsync(c->frame.counters, 0, sizeof(DevCounters), st));
  stageMark(c, st, "clear");

  launchInitPaths(c->scene.S, F, P, V, st);
  stageMark(c, st, "init_paths");

  // Both walks (eye vertices 2..D, BDPTMain.rt.hlsl:106-112; light vertices 1..D, :138-145) in one persistent
  // launch: traversal and hit/miss shading alternate inside the kernel, lanes re-arm themselves per bounce.
  launchWalk(c->scene.S, F, P, V, c->grids, c->numCUs, st);
  stageMark(c, st, "walk");

  // NEE terms (caller's stream) and splat terms (second stream) are generated side by side and traced at once (ray
  // class RAY_TERMS) while the connection generator — the long one — fills the RAY_PAIRS queue on the second stream;
  // the connection rays are traced when both are done.  (The MIS weights read both paths: everything sequential then.)
  const bool mis = (p->flags & (BDPT_PARAM_MIS_POWER | BDPT_PARAM_MIS_LINEAR)) != 0;
  if (mis) {
    launchMisPrefix(F, P, st);
    stageMark(c, st, "mis_prefix");
    launchGenNee(c->scene.S, F, PE, V.area, st);
    stageMark(c, st, "gen_nee");
    launchGenSplat(c->scene.S, F, P, st);
    stageMark(c, st, "gen_splat");
    launchGenConnect(c->scene.S, F, PE, st);
    stageMark(c, st, "gen_connect");
    launchTraceShadow(c->scene.S, F, P, RAY_TERMS, c->grids, c->numCUs, st);
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
    launchGenSplat(c->scene.S, F, P, c->walkStream);  // beside the NEE generator; both are short and latency-bound
    sideEnd(c, c->walkStream);
    HIPCHK(c, hipEventRecord(c->evSplat, c->walkStream));
    sideBegin(c, c->walkStream, "side:gen_connect");
    launchGenConnect(c->scene.S, F, PE, c->walkStream);
    sideEnd(c, c->walkStream);
    HIPCHK(c, hipEventRecord(c->evJoin, c->walkStream));
    launchGenNee(c->scene.S, F, PE, V.area, st);
    stageMark(c, st, "gen_nee");
    HIPCHK(c, hipStreamWaitEvent(st, c->evSplat, 0));
    stageMark(c, st, "splat_wait");
    launchTraceShadow(c->scene.S, F, P, RAY_TERMS, c->grids, c->numCUs, st);
    stageMark(c, st, "trace_terms");
    HIPCHK(c, hipStreamWaitEvent(st, c->evJoin, 0));
    stageMark(c, st, "connect_wait");
  }
  launchTraceShadow(c->scene.S, F, P, RAY_PAIRS, c->grids, c->numCUs, st);
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
  if (c->groups.splat && c->groups.planes >= planes) return BDPT_OK;
  if (streamIsCapturing(st)) {
    fail(c, "light groups: the splat planes need bdpt_prepare(BDPT_PREPARE_LIGHT_GROUPS / _LIGHT_GROUP_TABLE) before stream capture");
    return BDPT_E_STATE;
  }
  if (c->groups.splat) {  // too few planes for this assignment: frames in flight still use them
    HIPCHK(c, hipDeviceSynchronize());
    dropLightGroups(c->groups);
  }
  const size_t n = (size_t)c->frame.W * c->frame.H;
  void *sp = nullptr, *li = nullptr;
  if (hipMalloc(&sp, std::max<size_t>((size_t)planes * n * 4 * sizeof(unsigned long long), 16)) != hipSuccess ||
      hipMalloc(&li, std::max<size_t>(c->frame.P.Np, 16)) != hipSuccess) {
    if (sp) (void)hipFree(sp);
    fail(c, "light groups: hipMalloc of the splat planes failed");
    return BDPT_E_NOMEM;
  }
  c->groups.splat = reinterpret_cast<unsigned long long*>(sp);
  c->groups.planes = planes;
  c->groups.lightIdx = reinterpret_cast<uint8_t*>(li);
  return BDPT_OK;
}

// What bdpt_execute_light_groups, bdpt_execute_masked and the adaptive calls refuse alike, as "<what>: ...": the deferred
// stages (when params are given), a context without scene or size, and one that does not render the whole frame.
int wholeFrameCheck(bdpt_ctx* c, const bdpt_params* p, const std::string& what) {
  if (p && (p->flags & (BDPT_PARAM_DEFER_RESOLVE | BDPT_PARAM_DEFER_TAIL))) {
    fail(c, what + ": BDPT_PARAM_DEFER_RESOLVE and BDPT_PARAM_DEFER_TAIL are not supported");
    return BDPT_E_INVALID;
  }
  if (!c->scene.have || !c->frame.have) {
    fail(c, what + ": scene and size must be set first");
    return BDPT_E_STATE;
  }
  if (c->frame.tile.stripes.stripeRows != 0 || c->frame.tile.rows != c->frame.H) {
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
  if (!groups) return refuse(c, BDPT_E_INVALID, "light groups", "groups is NULL");
  if (int rc = wholeFrameCheck(c, p, "light groups")) return rc;
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = allocLightGroups(c, st, c->scene.S.numLights)) return rc;
  FrameVariant V;  // the identity assignment: group k = light k
  V.kind = FrameKind::Groups;
  V.groups.planes = groups;
  V.groups.splat = c->groups.splat;
  V.groups.lightIdx = c->groups.lightIdx;
  V.groups.numLights = c->scene.S.numLights;
  V.groups.numGroups = c->scene.S.numLights;
  V.groups.framePix = (uint64_t)c->frame.W * c->frame.H;
  for (uint32_t i = 0; i < c->scene.S.numLights; i++) V.groups.groupOf[i] = (uint8_t)i;
  return executeFrame(c, p, in, out, stream, V);
}

int bdpt_execute_grouped(bdpt_ctx* c, const bdpt_params* p, const bdpt_gbuffer* in, float* out, const bdpt_light_group_desc* d,
                         void* stream) {
  if (!c) return BDPT_E_INVALID;
  if (!p || !out) return refuse(c, BDPT_E_INVALID, "execute_grouped", "params or out is NULL");
  if (!d || !d->planes || !d->groupOf) return refuse(c, BDPT_E_INVALID, "execute_grouped", "the descriptor, its planes or its groupOf is NULL");
  if (int rc = wholeFrameCheck(c, p, "execute_grouped")) return rc;
  if (d->numGroups < 1 || d->numGroups > BDPT_MAX_LIGHTS + 1) {
    fail(c, "execute_grouped: numGroups must be 1 .. BDPT_MAX_LIGHTS + 1");
    return BDPT_E_INVALID;
  }
  const bool area = (p->flags & BDPT_PARAM_AREA_LIGHTS) != 0;
  const uint32_t numLights = c->scene.S.numLights;
  if (d->numAssigned != numLights + (area ? 1u : 0u)) {
    fail(c, "execute_grouped: numAssigned must be numLights, or numLights + 1 with BDPT_PARAM_AREA_LIGHTS");
    return BDPT_E_INVALID;
  }
  for (uint32_t i = 0; i < d->numAssigned; i++)
    if (d->groupOf[i] >= d->numGroups) {
      fail(c, "execute_grouped: groupOf[" + std::to_string(i) + "] is not below numGroups");
      return BDPT_E_INVALID;
    }
  if (d->reserved[0] || d->reserved[1]) return refuse(c, BDPT_E_INVALID, "execute_grouped", "reserved must be 0");
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
  V.groups.splat = c->groups.splat;
  V.groups.lightIdx = c->groups.lightIdx;
  V.groups.numLights = numLights;
  V.groups.numGroups = d->numGroups;
  V.groups.framePix = (uint64_t)c->frame.W * c->frame.H;
  for (uint32_t i = 0; i < d->numAssigned; i++) V.groups.groupOf[i] = d->groupOf[i];
  return executeFrame(c, p, in, out, stream, V, true);
}

int bdpt_execute_masked(bdpt_ctx* c, const bdpt_params* p, const bdpt_gbuffer* in, const uint8_t* mask, float* out, void* stream) {
  if (!c) return BDPT_E_INVALID;
  if (!mask) return refuse(c, BDPT_E_INVALID, "execute_masked", "mask is NULL");
  if (int rc = wholeFrameCheck(c, p, "execute_masked")) return rc;
  // The eye list: the active valid pixels, which init_paths pushes (where it lives: kEyeCountBlock).  Under MIS the walk's
  // eye lists stay the valid list: every valid pixel's eye prefix products are read by its splats.
  const PathBuf& P = c->frame.P;
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
  A.W = c->frame.W;
  A.H = c->frame.H;
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
  if (!a || !frame) return refuse(c, BDPT_E_INVALID, "adaptive_update", "params or frame is NULL");
  const uint32_t b = a->blockSize;
  if (b != 1 && b != 2 && b != 4 && b != 8 && b != 16) return refuse(c, BDPT_E_INVALID, "adaptive_update", "blockSize must be 1, 2, 4, 8 or 16");
  if (a->minSamples < 2 || a->maxSamples < a->minSamples) return refuse(c, BDPT_E_INVALID, "adaptive_update", "need 2 <= minSamples <= maxSamples");
  if (reinterpret_cast<uintptr_t>(frame) % 16 != 0) return refuse(c, BDPT_E_INVALID, "adaptive_update", "frame must be 16-byte aligned (RGBA32F)");
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
    if (!c->frame.have) return refuse(c, BDPT_E_STATE, "prepare", "bdpt_resize must be called first");
  }
  if ((what & (BDPT_PREPARE_REFIT | BDPT_PREPARE_REFIT_PIECES)) && !c->scene.have) {
    fail(c, "prepare: BDPT_PREPARE_REFIT needs a scene");
    return BDPT_E_STATE;
  }
  if ((what & BDPT_PREPARE_AREA_LIGHTS) && !c->scene.have) return refuse(c, BDPT_E_STATE, "prepare", "BDPT_PREPARE_AREA_LIGHTS needs a scene");
  if ((what & BDPT_PREPARE_MOTION) && !c->scene.have) return refuse(c, BDPT_E_STATE, "prepare", "BDPT_PREPARE_MOTION needs a scene");
  if ((what & (BDPT_PREPARE_LIGHT_GROUPS | BDPT_PREPARE_LIGHT_GROUP_TABLE)) && !c->scene.have) {
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
    if (int rc = ensureBmfrHistory(c, c->frame.bmfr, 1, nullptr, "bmfr", kBmfrPrepare)) return rc;
  if (what & (BDPT_PREPARE_LIGHT_GROUPS | BDPT_PREPARE_LIGHT_GROUP_TABLE))  // (_TABLE: a plane for the emitter table's group too)
    if (int rc = allocLightGroups(c, nullptr, c->scene.S.numLights + ((what & BDPT_PREPARE_LIGHT_GROUP_TABLE) ? 1u : 0u))) return rc;
  if (what & BDPT_PREPARE_AREA_LIGHTS)
    if (int rc = ensureAreaLights(c, nullptr)) return rc;
  if (what & BDPT_PREPARE_MOTION)
    if (int rc = allocPrevPose(c)) return rc;
  return BDPT_OK;
}

int bdpt_tile_pack(bdpt_ctx* c, const void* frame, void* packed, uint32_t bytesPerPixel, void* stream) {
  if (!c || !frame || !packed || (bytesPerPixel != 4 && bytesPerPixel != 8 && bytesPerPixel != 16)) return BDPT_E_INVALID;
  if (!c->frame.have) return BDPT_E_STATE;
  ENTER(c);
  launchTilePack(frame, packed, bytesPerPixel, c->frame.P.pix, c->frame.P.Np, reinterpret_cast<hipStream_t>(stream));
  HIPCHK(c, hipGetLastError());
  return BDPT_OK;
}
int bdpt_tile_unpack(bdpt_ctx* c, uint32_t owner, const void* packed, void* frame, uint32_t bytesPerPixel, void* stream) {
  if (!c || !frame || !packed || (bytesPerPixel != 4 && bytesPerPixel != 8 && bytesPerPixel != 16)) return BDPT_E_INVALID;
  if (!c->frame.have) return BDPT_E_STATE;
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (c->frame.tile.stripes.stripeRows == 0) {  // a band: its rows are one run
    if (owner != 0) return BDPT_E_INVALID;
    if (c->frame.tile.rows)
      HIPCHK(c, hipMemcpyAsync(static_cast<uint8_t*>(frame) + (size_t)c->frame.tile.rowRanges.front().first * c->frame.W * bytesPerPixel, packed,
                               (size_t)c->frame.tile.rows * c->frame.W * bytesPerPixel, hipMemcpyDeviceToDevice, st));
    return BDPT_OK;
  }
  if (owner >= c->frame.tile.stripes.numOwners) return BDPT_E_INVALID;
  const TileDesc& t = c->frame.tile;
  launchTileUnpack(packed, frame, bytesPerPixel, c->frame.W, c->frame.H, t.stripes.stripeRows, t.stripes.numOwners, owner, t.sl.chunkRows, st);
  HIPCHK(c, hipGetLastError());
  return BDPT_OK;
}

int bdpt_splat_buffer(bdpt_ctx* c, uint64_t** out_ptr, uint64_t* out_n) {
  if (!c || !out_ptr) return BDPT_E_INVALID;
  if (!c->frame.have) return BDPT_E_STATE;
  *out_ptr = reinterpret_cast<uint64_t*>(c->frame.splat);
  if (out_n) *out_n = (uint64_t)c->frame.tile.sl.owners * c->frame.tile.sl.chunkRows * c->frame.W * 4;
  return BDPT_OK;
}

int bdpt_set_splat_buffer(bdpt_ctx* c, uint64_t* device_ptr, uint64_t num_u64) {
  if (!c) return BDPT_E_INVALID;
  if (!c->frame.have) return BDPT_E_STATE;
  if (!device_ptr) {
    c->frame.splat = c->frame.ownSplat;
    return BDPT_OK;
  }
  if (num_u64 < (uint64_t)c->frame.tile.sl.owners * c->frame.tile.sl.chunkRows * c->frame.W * 4) {
    fail(c, "set_splat_buffer: buffer smaller than bdpt_get_tile_info's splatU64");
    return BDPT_E_INVALID;
  }
  c->frame.splat = reinterpret_cast<unsigned long long*>(device_ptr);
  return BDPT_OK;
}

int bdpt_resolve(bdpt_ctx* c, const uint64_t* splat, uint32_t splat_row0, float* out, void* stream) {
  if (!c || !splat || !out) return BDPT_E_INVALID;
  if (!c->frame.have) return BDPT_E_STATE;
  const uint32_t firstRow = c->frame.tile.rowRanges.empty() ? 0 : c->frame.tile.rowRanges.front().first;
  if (splat_row0 > firstRow || (splat_row0 != 0 && c->frame.tile.sl.owners != 1)) {
    fail(c, "resolve: splat buffer does not cover the tile");
    return BDPT_E_INVALID;
  }
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  launchResolve(reinterpret_cast<const unsigned long long*>(splat), false, splat_row0, c->frame.tile.sl, out, c->frame.W, c->frame.P.pix, c->frame.P.Np, st);
  HIPCHK(c, hipGetLastError());
  return BDPT_OK;
}

int bdpt_resolve_tile(bdpt_ctx* c, const uint64_t* tile_splat, float* out, void* stream) {
  if (!c || !tile_splat || !out) return BDPT_E_INVALID;
  if (!c->frame.have) return BDPT_E_STATE;
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  launchResolve(reinterpret_cast<const unsigned long long*>(tile_splat), true, 0, c->frame.tile.sl, out, c->frame.W, c->frame.P.pix, c->frame.P.Np, st);
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
  if (!c->frame.have) return BDPT_E_STATE;
  ENTER(c);
  launchAccumulateTile(lastFrame, curFrame, accumCount, maxAccumCount, c->frame.P.pix, c->frame.P.Np, reinterpret_cast<hipStream_t>(stream));
  HIPCHK(c, hipGetLastError());
  return BDPT_OK;
}

}  // extern "C"
