// kernels.h — device-side views and launch entry points shared by kernels.hip and the entry points (api*.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bdpt.h"
#include "texture_planes.h"

namespace bdpt {

constexpr int kWave = 64;          // gfx950 wavefront
#ifndef KSTACK
#define KSTACK 32
#endif
constexpr int kStackEntries = KSTACK;  // per-lane traversal stack capacity (the builder's bound is kBvhMaxStack = KSTACK - 1)
// The any-hit kernel keeps only the first BDPT_STACK_LDS entries of a lane's stack in LDS (6 KiB per wave); the few
// deeper entries of very deep descents go to a per-context overflow area in device memory (SceneDev::stackOvf).
// Measured on the bench frame: rays never go beyond 12 entries there, and the smaller LDS footprint (more resident
// any-hit waves, room for the connection generator beside them) is worth 3 % of the frame (profiles/README.md).
#ifndef BDPT_STACK_LDS
#define BDPT_STACK_LDS 24
#endif
constexpr int kStackLds = BDPT_STACK_LDS < KSTACK ? BDPT_STACK_LDS : KSTACK;
// The walk kernel keeps BDPT_WALK_STACK_LDS rows in LDS and the rest in the same overflow area: four rows of a wave are
// exactly the 1 KiB its sRGB table takes (kernels.hip walk_kernel), so its LDS footprint stays 10 KiB per wave.
#ifndef BDPT_WALK_STACK_LDS
#define BDPT_WALK_STACK_LDS 28
#endif
constexpr int kWalkStackLds = BDPT_WALK_STACK_LDS < KSTACK ? BDPT_WALK_STACK_LDS : KSTACK;
constexpr int kMaxPersistentPerCU = 32;  // resident one-wave workgroups per CU a persistent grid may use (8 per SIMD)
// Rows of the per-context stack overflow area (SceneDev::stackOvf).  INVARIANT the area relies on: it is indexed by
// workgroup and lane only, so no two persistent traversal launches of one context may be resident at once — every
// launchWalk / launchTraceShadow of a context goes to the caller's stream, the context's second stream only runs
// generators (api_frame.cpp bdpt_execute, evFork / evJoin), the test hooks synchronise the device first, and launchTraceRays
// (bdpt_trace_rays) goes to the caller's stream ordered behind everything the context's previous call enqueued.
// Rows: what the kernel with the fewest LDS rows needs (each indexes its own entry - rows-in-LDS from row 0).
constexpr int kStackOvfRows = KSTACK - (kStackLds < kWalkStackLds ? kStackLds : kWalkStackLds);
constexpr int kShadeRecF4 = 8;  // float4s per triangle shading record: 7 used (112 B), the eighth zero, so that a record is one 128-byte line
constexpr uint32_t kNoRay = 0xFFFFFFFFu;
// Hot single-word atomics top out near 90 M/s on this chip (MI355X_MICROARCH.md "dequeue"), so
// producer and consumer cursors of every queue are sharded over sub-queues, the any-hit trace kernel
// takes up to kFetchChunk rays per atomic, and the statistics counters are sharded per workgroup.
constexpr uint32_t kNumSubQueues = 32;
#ifndef BDPT_FETCH_CHUNK
#define BDPT_FETCH_CHUNK 256
#endif
constexpr uint32_t kFetchChunk = BDPT_FETCH_CHUNK;
constexpr uint32_t kCursorStride = 32;                            // uint32 words between two sub-queue cursors: one 128-byte line each
constexpr uint32_t kCursorBlock = kNumSubQueues * kCursorStride;  // words of one sharded cursor
// The ray queues have their own cursor count (BDPT_RAY_SUBQUEUES).  Measured on the bench frame: 128 cursors instead
// of 32 change nothing (20.9 vs 20.5 ms: the appends of the generators are not what bounds them).
#ifndef BDPT_RAY_SUBQUEUES
#define BDPT_RAY_SUBQUEUES 32
#endif
constexpr uint32_t kNumRaySubQueues = BDPT_RAY_SUBQUEUES;
constexpr uint32_t kRayCursorBlock = kNumRaySubQueues * kCursorStride;  // words of one sharded ray cursor
constexpr uint32_t kCounterShards = 64;

// Path-vertex field ids (PathVertex, BDPT/RayPathData.hlsli:1-45); kernels.hip "Path vertices" maps them to the 96-byte record.  pdfForward is only read by the
// MIS weights (BDPT_PARAM_MIS_*), which the reference defines but never calls.
enum : int { F_COL = 0, F_POS = 3, F_N = 6, F_V = 9, F_DIF = 12, F_SPEC = 15, F_ROUGH = 18, F_ISSPEC = 19, F_PDF = 20, NF = 21 };
constexpr int NF4 = 6;  // float4s per stored vertex record (96 B; layout in kernels.hip "Path vertices")
enum : int { PATH_EYE = 0, PATH_LIGHT = 1 };
enum : int { RAY_TERMS = 0, RAY_PAIRS = 1 };

// pow2: texPow2Flags (texture_planes.h: bit 0 set when w is a power of two, bit 1 when h is; wrapT wraps by mask there)
struct TexDev {
  const uint8_t* px;
  uint32_t w, h, srgb, pow2;
};

struct SceneConst {
  bdpt_light lights[BDPT_MAX_LIGHTS];
  float srgbLut[256];
};

struct SceneDev {
  const uint4* recs;        // 3 per 48-byte record: interior nodes and leaf triangles in one array (bvh.h BvhRec)
  const float4* shade;      // kShadeRecF4 per primitive, primitive order
  const float* bitangents;  // 3 per vertex (normal-mapped primary hits only)
  const uint32_t* indices;  // 3 per primitive
  const bdpt_material* materials;
  const TexDev* textures;
  const TexDev* matTex;     // 4 per material: descriptors of its base-colour, specular, emissive and normal textures (zero when absent)
  const SceneConst* sc;
  uint32_t numLights;
  uint32_t hasBitangents;
  uint32_t numRecs;
  const float4* alphaRecs;  // 4 per non-opaque triangle (device_scene.hpp alphaTestFails), indexed by BvhTri::aux
  int* stackOvf;            // overflow rows of the persistent kernels' stacks: [entry - rows in LDS][workgroup * 64 + lane]
  uint32_t stackOvfStride;  // lanes per row
  // occluder hints for next-event rays (kernels.hip "Occluder hints"): per point / spot light a cube map of the record
  // index of the nearest triangle in each direction from the light; [light][face][v][u], kNoHint where nothing is seen
  const uint32_t* lightMap;
  uint32_t lightMapRes;     // texels per cube-face edge (0: no maps)
};

struct DevCounters {  // [shard][field]; fields mirror bdpt_counters; two 128-byte lines per shard
  unsigned long long v[kCounterShards][32];
};
enum : int {
  C_RAYS_PRIMARY = 0, C_RAYS_EYE, C_RAYS_LIGHT, C_RAYS_NEE, C_RAYS_SPLAT, C_RAYS_CONNECT,
  C_NODE_CLOSEST, C_TRI_CLOSEST, C_NODE_SHADOW, C_TRI_SHADOW, C_PIX_VALID, C_SPLATS, C_RAYS_LAZY,
  C_STACK_MAX,  // deepest any-hit traversal stack seen (a maximum, not a sum; with BDPT_PARAM_COUNTERS)
  C_ALPHA_CLOSEST, C_ALPHA_SHADOW,  // any-hit alpha tests run by closest-hit / any-hit queries (with BDPT_PARAM_COUNTERS)
  C_HINT_NEE, C_HINT_SPLAT          // any-hit queries answered "occluded" by their occluder hint (not part of C_RAYS_*)
};

// Number of connection pairs the reference defines for depth D (cameraLength <= totalLength,
// BDPTMain.rt.hlsl:212-216): sum_{t=2..D} min(t, D-1).
inline __host__ __device__ uint32_t numConnectPairs(uint32_t D) {
  uint32_t n = 0;
  for (uint32_t t = 2; t <= D; t++) n += (t < D - 1) ? t : (D - 1);
  return n;
}

// Per-tile path state, SoA by tile-local pixel index p in [0, Np).
struct PathBuf {
  float* v;            // vertex records: ((path*D1 + k)*Np + p) * NF4 float4s
  float* rayDir;       // planes: (path*3 + axis)*Np + p
  const uint32_t* pix; // tile-local pixel p -> full-frame pixel index y*W + x (the tile's rows, row-major)
  // RNG state after sampleLight, where gen_nee's, the gather's and light_query's draws start.  The walks do not read it: the
  // state a sub-path draws from travels in q0.w of its vertex records (kernels.hip "Path vertices"), the eye walk's too
  uint32_t* seedL;
  uint8_t* eyeLast;    // last stored eye vertex (ghost included); 0 = pixel has no geometry
  uint8_t* lightLast;  // last stored light vertex (ghost included)
  uint8_t* lightReal;  // number of light vertices produced by hits (takeContribution, BDPTMain.rt.hlsl:144)
  uint32_t* queue[3];  // sharded pixel queues (kernels.hip "Path queues"): [0] valid pixels; [1],[2] lazy-round ping-pong
  uint32_t pathSubCap; // capacity of one list of a path queue (multiple of 64)
  // cursor blocks: each is kNumSubQueues cursors, one per 128-byte line (kCursorBlock words)
  uint32_t* qcount;    // block 0 = valid-pixel list lengths
  uint32_t* qhead;     // blocks 0-1 = fetch cursors of the walk kernel (one per virtual list: pixel list x path)
  // shadow-ray queue (NEE + splat + connection rays of one frame)
  float* rayQ;           // 7 planes, stride rayCap
  float* rayContrib;     // 3 planes, stride rayCap: the clamped contribution the ray gates
  uint8_t* rayVis;       // visibility by ray id
  // Two ray classes share the planes: RAY_TERMS (NEE + splat rays) and RAY_PAIRS (connection rays, lazy rounds), each
  // with its own sub-queues and cursors, so the first can be traced while the second is still being generated.
  uint32_t* rayCount;    // cursor blocks [class]: rays queued per sub-queue
  uint32_t* rayHead;     // cursor blocks [class]: fetch cursors
  uint32_t raySubCap[2]; // capacity of one sub-queue of the class
  uint32_t rayBase[2];   // first ray id of the class; ray id = rayBase[c] + subQueue*raySubCap[c] + offset
  uint32_t* slotRay;     // planes: slot*Np + p -> ray id or kNoRay.  slots: [0,D) NEE, [D,2D) splat, [2D,..) pairs
  uint32_t* splatPix;    // planes: t*Np + p -> full-frame pixel index of splat t
  float* misE;           // planes: k*Np + p, k in [0, D]: eye-side prefix product of getWeightPower/Linear
  float* misL;           // same, light side
  uint8_t* lazyCursor;   // next connection-pair ordinal a pending pixel has not examined yet
  uint32_t* lazyRay;     // planes: b*Np + p -> ray id of the b-th lazy ray of the current round
  uint32_t* lazyCount;   // cursor blocks: pending-list lengths, one block per round
  uint32_t rayCap;
  uint32_t Np, D1;
};

// Where a frame pixel's splat accumulator lives: owner-major, so that one reduce-scatter over ranks hands every
// rank the accumulators of its own rows as one contiguous chunk.  Rows are dealt to `owners` ranks in stripes of
// `stripeRows`; owner o's chunk holds its rows in order, padded to chunkRows.  owners == 1 is plain frame order.
struct SplatLayout {
  uint32_t stripeRows, owners, chunkRows;
};
inline __host__ __device__ size_t splatIndex(const SplatLayout& L, uint32_t W, uint32_t x, uint32_t y) {
  const uint32_t s = y / L.stripeRows;
  const uint32_t owner = s % L.owners, row = (s / L.owners) * L.stripeRows + (y - s * L.stripeRows);
  return ((size_t)owner * L.chunkRows + row) * W + x;
}

struct FrameDev {
  bdpt_camera cam;
  bdpt_params p;
  uint32_t W, H;
  SplatLayout sl;
  float* out;                 // full-frame RGBA32F
  unsigned long long* splat;  // 4 x u64 per pixel, SplatLayout order
  bdpt_gbuffer gb;
  DevCounters* counters;
  // environment of the BDPT pass (BDPT_PARAM_ENV_ON_MISS; bdpt_set_environment): RGBA32F lat-long map or constant colour
  const float* envMap;
  uint32_t envW, envH;
  float envColor[3];
  // occluder hints for light-tracing rays: record index of the triangle the primary ray of each FRAME pixel hit
  // (written by the context's own G-buffer pass; kNoHint where it has not run or saw nothing); NULL = no hints
  const uint32_t* hintPix;
};

// Light groups (bdpt_execute_light_groups, bdpt_execute_grouped): one RGBA32F plane per group of lights plus one for
// emission, from the paths of the plain frame.  A term's source light (the emitter table is light numLights) decides its
// plane through `groupOf`; bdpt_execute_light_groups is the identity assignment.  The group instances of init_paths, gather
// and lazy_check and the group resolve take it (FrameVariant).  The assignment travels by value in the kernel argument, so
// a captured graph holds it.  Whole-frame contexts only: planes and splat planes are indexed by frame pixel (splat planes
// in SplatLayout order, which is frame order there).
struct GroupDev {
  float* planes;               // (numGroups + 1) planes of W*H float4: plane g < numGroups = group g, plane numGroups = emission
  unsigned long long* splat;   // numGroups splat-value planes of W*H x 4 u64 (r, g, b, unused); counts stay in FrameDev::splat
  uint8_t* lightIdx;           // tile-local pixel p -> the light its light subpath starts at (init_paths); numLights = the table
  uint32_t numLights;
  uint32_t numGroups;
  uint64_t framePix;           // W*H: the stride of both kinds of plane
  const float* areaW;          // AreaDev::total (the table's W word) of a frame with BDPT_PARAM_AREA_LIGHTS and emitters, else NULL
  uint8_t groupOf[BDPT_MAX_LIGHTS + 1];  // light -> group; entry numLights = the emitter table
};

// Masked frames (bdpt_execute_masked): only the pixels a caller's mask selects trace eye paths, NEE and connection rays,
// gather and write `out`; every valid pixel still traces its light subpath and its splats.  The masked instances of
// init_paths, walk and gather and the masked resolve take it (FrameVariant); gen_nee, gen_connect and the lazy rounds
// run unchanged on a PathBuf copy whose queue[0] / qcount name the eye list.  Whole-frame contexts only (the mask is
// indexed by frame pixel).
struct MaskDev {
  const uint8_t* mask;          // W*H bytes, frame order: non-zero = active
  uint32_t* eye;                // eye list: the active valid pixels, sharded as PathBuf::queue[0] (init_paths appends)
  uint32_t* eyeCount;           // its cursor block (kCursorBlock words, zero when init_paths starts)
  const uint32_t* walkEye;      // what the walk's eye lists read: `eye`, or under MIS the valid list (PathBuf::queue[0])
  const uint32_t* walkEyeCount; // and their lengths
};

// Area lights (BDPT_PARAM_AREA_LIGHTS; contract in include/bdpt.h "Area lights"): the scene's emitting triangles in
// ascending primitive order and their selection CDF, built and refreshed on the device (area_lights.hip).  Only the AREA
// instances of init_paths and gen_nee take it (last argument), so SceneDev and every other instance stay as they are.
// (A group frame's gather re-forms the light count from GroupDev::areaW, the same word.)
constexpr uint32_t kNoAlphaRec = 0xFFFFFFFFu;
struct BvhRefitNode;  // bvh.h
struct AreaDev {
  const float* cdf;     // n inclusive prefix sums of the weights (fp32, fixed summation order)
  const float4* emit;   // per emitter: prim (bits), alpha-test record (bits, kNoAlphaRec when opaque), weight, area
  const float* total;   // two device words: W = cdf[n - 1], and the last emitter with a positive weight (bits)
  uint32_t n;           // emitters; 0 = the frame runs the plain instances
};

// Which frame the per-pixel stages render: bdpt_execute, bdpt_execute_light_groups or bdpt_execute_masked.  Each kind is
// a template argument of the init_paths, walk, gather and lazy_check kernels, which take what it needs (GroupDev,
// MaskDev, or an empty struct for the plain frame) as their LAST argument, so the plain instances keep the offsets of
// their other arguments.  A masked frame runs the plain lazy_check, a group frame the plain walk.
enum class FrameKind { Plain, Groups, Masked };
struct FrameVariant {
  FrameKind kind = FrameKind::Plain;
  GroupDev groups{};  // kind == Groups
  MaskDev mask{};     // kind == Masked
  AreaDev area{};     // area.n > 0: the AREA instances of init_paths and gen_nee (every kind)
};

struct GBufferDev {
  bdpt_camera cam;
  bdpt_gbuffer_params gp;
  uint32_t W, H, Np;
  const uint32_t* pix;  // the tile's pixels (PathBuf::pix)
  bdpt_gbuffer gb;
  DevCounters* counters;
  uint32_t* hintPix;    // FrameDev::hintPix, written here (may be NULL)
};

// BMFR denoise pass (bmfr.hip): numPlanes images over one G-buffer (one for bdpt_bmfr_execute / _motion).  History buffers
// come in ping-pong pairs: R = previous frame (read), W = this frame (written), so the reference's post-pass blits
// (DenoisePass.cpp:180-182, 194) cost no extra copy.  The images share frame, flags, matrix, features, the position / normal
// history, accept, prevPixel and prevPos.  Plane k's noisy and filtered history: side s of slot k at
// hist*[(2 * k + s) * W * H]; `read` is the side that holds the previous frame.  The pointers travel by value in the kernel
// argument.
struct BmfrDev {
  uint32_t W, H, frame;
  uint32_t full, doPre;
  float m[16];                 // prevViewProj, row-major
  const float4* curPos;        // WorldPosition
  const uint16_t* curNorm;     // WorldNormal (half4)
  const uint16_t* albedo;      // MaterialDiffuse (half4)
  const float4 *prevPosR, *prevNormR;
  float4 *prevPosW, *prevNormW;
  uint8_t* accept;             // BMFR_AcceptedBools
  uint32_t* prevPixel;         // BMFR_PrevFramePixel, RG16Float
  const float4* prevPos;       // where each pixel's surface point was last frame (PrevWorldPosition); NULL = curPos
  uint32_t numPlanes, read;
  float4* planes[BDPT_BMFR_MAX_PLANES];  // the channels being denoised, in/out
  float4 *histNoisy, *histFiltered;
};
// one launch per stage whatever numPlanes is
void launchBmfr(const BmfrDev& A, uint32_t flags, hipStream_t st);

// Motion (motion.hip, device_motion.hpp; contract in include/bdpt.h "Motion"): the previous pose, three float4 per
// primitive (the corners p0, p1, p2 in primitive order, w unused), and the G-buffer channel made from it.  Only the MOTION
// instance of gbuffer_kernel takes it (last argument), so SceneDev, GBufferDev and every other instance stay as they are.
struct MotionDev {
  const float4* prevPose;  // 3 per primitive
  float4* prevPosition;    // W*H texels, frame order: (where the pixel's surface point was, 1), zeros on a miss
};
// prevPose <- the corner positions of the current shading records (words r0.xyz, r2.xyz, r4.xyz)
void launchKeepPose(const float4* shade, uint32_t numTris, float4* prevPose, hipStream_t st);
// bdpt_motion_query: out[i] = (prevPosAtHit(hits[i]), 1), zeros for a miss or a prim outside the scene; count caps cap
void launchMotionQuery(const float4* prevPose, uint32_t numTris, const float4* hits, uint32_t cap, const uint32_t* count, float4* out,
                       hipStream_t st);

// launchers (kernels.hip)
void launchGBuffer(const SceneDev& S, const GBufferDev& G, hipStream_t st);
// bdpt_gbuffer_execute_motion: launchGBuffer plus M.prevPosition (G.counters unused)
void launchGBufferMotion(const SceneDev& S, const GBufferDev& G, const MotionDev& M, hipStream_t st);
// SceneDev::alphaRecs (4 float4 per non-opaque triangle, in the order of alphaTris) from the shading records and material tables
// quadByTex: per texture id the device address of its alpha-quad plane (texture_planes.h alphaQuadRows), 0 where it has none
void launchAlphaRecs(const SceneDev& S, const uint32_t* alphaTris, uint32_t n, const unsigned long long* quadByTex, float4* out, hipStream_t st);
// FrameDev::hintPix of EVERY frame pixel (G.Np = W * H; nothing else is written): partial-tile contexts, on a camera change
void launchHintFill(const SceneDev& S, const GBufferDev& G, hipStream_t st);
// SceneDev::lightMap of every point / spot light of the scene (res texels per face edge), closest-hit rays from the light
void launchLightMaps(const SceneDev& S, uint32_t* maps, uint32_t res, hipStream_t st);
// The per-pixel stages of a frame take its variant.  Groups: init_paths also records each pixel's light and starts the
// background pixels' planes, gather / lazy_check also keep the planes, and the resolve does out and every plane in one
// pass (out's splat values are the sums of the per-light splat planes: FrameDev::splat then only holds the counts).
// Masked: init_paths also builds the eye list and writes `out` for active pixels only, the walk's eye lists read
// MaskDev::walkEye (and it adds ENV_ON_MISS / EMISSIVE_HITS terms to active pixels only), gather runs over every valid
// pixel but sums and writes only active ones (every pixel's splats still land), and the resolve does active pixels.
void launchInitPaths(const SceneDev& S, const FrameDev& F, const PathBuf& P, const FrameVariant& V, hipStream_t st);
// Persistent-grid sizes of one context's device, filled on first use (occupancy query per kernel variant).
struct LaunchGrids {
  uint32_t walk[16] = {};             // [MASKED][EXT][GGX][COUNT]
  uint32_t shadow[2] = {0, 0};        // [COUNT]
  uint32_t rays[3] = {0, 0, 0};       // [mode] (trace_rays.hip)
  uint32_t walkQuery[2] = {0, 0};     // [GGX] (walk_query.hip)
  uint32_t ao[2] = {0, 0};            // [G-buffer source] (ao.hip)
  uint32_t gi[3] = {0, 0, 0};         // [records, records + normal map, G-buffer] (gi.hip)
  uint32_t direct[4] = {0, 0, 0, 0};  // [G-buffer source][HINTS] (direct.hip)
  uint32_t sky[2] = {0, 0};           // [G-buffer source] (sky.hip)
  uint32_t skyMis[4] = {0, 0, 0, 0};  // [G-buffer source][GGX] (sky_mis.hip)
  uint32_t ris[16] = {};              // [G-buffer source][GGX][AREA][HINTS] (ris.hip)
  uint32_t reuse[8] = {};             // [G-buffer source][GGX][AREA] (reuse.hip)
};
// both random walks of the frame: one persistent launch (trace + hit/miss shading in place)
void launchWalk(const SceneDev& S, const FrameDev& F, const PathBuf& P, const FrameVariant& V, LaunchGrids& G, int numCUs,
                hipStream_t st);
void launchMisPrefix(const FrameDev& F, const PathBuf& P, hipStream_t st);
// A.n > 0: the AREA instance (area-light terms); otherwise the plain one
void launchGenNee(const SceneDev& S, const FrameDev& F, const PathBuf& P, const AreaDev& A, hipStream_t st);
void launchGenSplat(const SceneDev& S, const FrameDev& F, const PathBuf& P, hipStream_t st);
void launchGenConnect(const SceneDev& S, const FrameDev& F, const PathBuf& P, hipStream_t st);
void launchTraceShadow(const SceneDev& S, const FrameDev& F, const PathBuf& P, int rayClass, LaunchGrids& G, int numCUs, hipStream_t st);
// bdpt_trace_rays (trace_rays.hip): `cap` bdpt_ray records (two float4 each), of which the first min(*count, cap) are
// traced when `count` is set; mode 0 / 1 write bdpt_hit records (one float4 each) to `hits`, mode 2 visibility bytes to
// `vis`.  `cursor` (two words of the context, zeroed by bdpt_create) must be zero when the launch starts; the launch leaves
// it zero.
void launchTraceRays(const SceneDev& S, const float4* rays, uint32_t cap, const uint32_t* count, unsigned long long* cursor, int mode,
                     float4* hits, uint8_t* vis, LaunchGrids& G, int numCUs, hipStream_t st);
// surface_query.hip: bdpt_camera_rays (W * H rays), bdpt_shade_hits (six float4 per hit), bdpt_bsdf_query (SAMPLE: two float4
// per item, EVAL: one); count (optional device word) caps cap
void launchCameraRays(const bdpt_camera& cam, const bdpt_gbuffer_params& gp, uint32_t W, uint32_t H, float4* rays, hipStream_t st);
void launchShadeHits(const SceneDev& S, uint32_t numTris, const float4* rays, const float4* hits, uint32_t cap, const uint32_t* count,
                     bool normalMap, float4* out, hipStream_t st);
void launchBsdfQuery(const float4* surf, uint32_t cap, const uint32_t* count, bool eval, bool ggx, bool fromLobe, const uint32_t* seeds,
                     const float4* dirs, float4* out, hipStream_t st);
// What the per-item queries share (device_query.hpp reads them): the items of a launch and the dense ray list.
struct QueryRange {
  uint32_t cap;           // items; the capacity when count is set
  const uint32_t* count;  // optional device word: min(*count, cap) items
  float minT;             // tmin of the rays
};
struct CompactList {
  float4* rays;     // optional: dense list of the rays worth tracing (capacity: the query's cap)
  uint32_t* items;  //   their item indices
  uint32_t* count;  //   the list's length (the caller zeroes it)
};
// light_query.hip: bdpt_light_query.  NEE: one bdpt_light_sample (three float4) per bdpt_surface record and seed, and with
// compactRays the rays worth tracing appended to a dense list; EMIT: one bdpt_light_emit (three float4) per seed.
struct LightQueryDev {
  const float4* surf;      // NEE: bdpt_surface records (six float4 each)
  const uint32_t* seeds;   // one RNG state per item
  uint32_t* seedsOut;      // optional: NEE the state after the selection draw, EMIT the state after all draws (seedL)
  float4* out;             // three float4 per item
  QueryRange range;        // minT: also of the occluder-hint test
  CompactList compact;     // NEE, optional: the rays with status == NONZERO
};
// A.n > 0: the AREA instances (the emitter table is light numLights while its W is positive)
void launchLightQuery(const SceneDev& S, const LightQueryDev& Q, const AreaDev& A, bool emitMode, bool ggx, bool hints, hipStream_t st);
// connect_query.hip: bdpt_connect_query.  VERTICES: one bdpt_connect_sample (three float4) per pair of bdpt_surface records;
// CAMERA: one bdpt_camera_sample (four float4) per record; with compactRays the rays worth tracing go to a dense list.
struct ConnectQueryDev {
  const float4* eye;             // VERTICES: bdpt_surface records (six float4 each)
  const float4* light;           // both modes
  const float4* eyePrev;         // VERTICES, optional: the predecessors' positions (xyz of a float4)
  const float4* lightPrev;
  const uint8_t* eyeSpecular;    // optional: bdpt_bsdf_sample::specular of the vertex (NULL = 0)
  const uint8_t* lightSpecular;
  float4* out;                   // three (VERTICES) or four (CAMERA) float4 per item
  QueryRange range;
  uint32_t width, height;        // CAMERA: the frame
  float jitter[2];               // CAMERA: bdpt_params::pixelJitter
  CompactList compact;           // optional: the rays with NONZERO (VERTICES) / PIXEL (CAMERA)
};
// cam: the context's camera for CAMERA mode, nullptr for VERTICES
void launchConnectQuery(const ConnectQueryDev& Q, const bdpt_camera* cam, bool ggx, hipStream_t st);
// bdpt_splat_add: entry j adds values[k] to splat[pixels[k]], k = items ? items[j] : j, when visible[j] (or no visible)
struct SplatAddDev {
  const uint32_t* pixels;
  const float4* values;
  const uint8_t* visible;  // optional
  const uint32_t* items;   // optional
  unsigned long long* splat;
  uint32_t numPixels;
  uint32_t cap;
  const uint32_t* count;   // optional device word
};
void launchSplatAdd(const SplatAddDev& A, hipStream_t st);
// walk_query.hip: bdpt_walk_query.  One subpath per item, up to `steps` bounces: plane s of item i is element s * cap + i
// of vertices (six float4), info (one), samples (two) and hits (one).
struct WalkQueryDev {
  const float4* starts;          // three float4 per item: (org, tmin) (dir, tmax) (colour, unused)
  const uint32_t* seeds;         // cap states, or steps x cap with seedPerStep
  const float4* first;           // optional: bdpt_surface records, the predecessor a step-0 ghost copies (its posW is the origin)
  const uint8_t* firstSpecular;  // optional
  const uint8_t* alive;          // optional: 0 = no path
  float4* vertices;
  float4* info;
  float4* samples;               // optional
  float4* hits;                  // optional
  QueryRange range;              // minT: tmin of the rays after step 0
  uint32_t steps;
  uint32_t seedPerStep;
};
// `cursor`: as launchTraceRays (the context's two words: zero when the launch starts, left zero)
void launchWalkQuery(const SceneDev& S, const WalkQueryDev& Q, bool ggx, bool fromLobe, unsigned long long* cursor, LaunchGrids& G,
                     int numCUs, hipStream_t st);
// ao.hip: bdpt_ao_query (items are bdpt_surface records) and bdpt_ao_execute (items are the tile's pixels, read from the
// G-buffer).  `samples` any-hit rays per alive item from its position inside (range.minT, radius).
struct AoDev {  // fields without a comment: the item source (device_item_source.hpp)
  const float4* surf;        // posW, N and prim are read
  const uint32_t* seeds;
  const uint8_t* alive;
  float* ao;                 // query: count / samples per item
  uint32_t* counts;          // query, optional: unoccluded samples per item
  uint32_t* seedsOut;        // query, optional: the state after 2 * samples draws (a dead item's: unchanged)
  const float4* gbPosition;
  const uint16_t* gbNormal;
  const uint32_t* pix;
  float4* out;               // execute: (ao, ao, ao, 1) at the tile's pixels
  QueryRange range;
  float radius;              // tmax of the rays
  uint32_t samples;          // 1 .. 64
  uint32_t frameCount;       // execute
};
// `cursor`: as launchTraceRays (the context's two words: zero when the launch starts, left zero)
void launchAo(const SceneDev& S, const AoDev& A, bool gbuffer, unsigned long long* cursor, LaunchGrids& G, int numCUs, hipStream_t st);
// gi.hip: bdpt_gi_query (items are bdpt_surface records) and bdpt_gi_execute (items are the tile's pixels, read from the
// G-buffer).  Per alive item a direct any-hit ray, and with BDPT_GI_INDIRECT a closest-hit bounce ray and an any-hit ray
// from its hit.
struct GiDev {  // fields without a comment: the item source (device_item_source.hpp)
  const float4* surf;         // posW, N, diffuse and prim are read
  const uint32_t* seeds;
  const uint8_t* alive;
  float4* color;
  float4* hits;               // query, optional: the bounce ray's bdpt_hit
  uint32_t* status;           // query, optional: BDPT_GI_STATUS_*
  uint32_t* seedsOut;         // query, optional: the state after 1 or 3 draws (a dead item's: unchanged)
  const float4* gbPosition;
  const uint16_t* gbNormal;
  const uint16_t* gbDiffuse;
  const uint32_t* pix;
  float4* out;
  QueryRange range;
  uint32_t flags;             // BDPT_GI_INDIRECT | BDPT_GI_UNIFORM | BDPT_GI_SHADE_FROM_VIEW
  uint32_t frameCount;        // execute
  float viewPos[3];           // BDPT_GI_SHADE_FROM_VIEW: where the bounce hit is shaded from
  const float* envMap;        // the context's environment (bdpt_set_environment): RGBA32F map, or null: envColor
  uint32_t envW, envH;
  float envColor[3];
};
// `cursor`: as launchTraceRays (the context's two words: zero when the launch starts, left zero)
void launchGi(const SceneDev& S, const GiDev& Q, bool gbuffer, bool normalMap, unsigned long long* cursor, LaunchGrids& G, int numCUs,
              hipStream_t st);
// direct.hip: bdpt_direct_query (items are bdpt_surface records) and bdpt_direct_execute (items are the tile's pixels, read
// from the G-buffer).  Per alive item and light of the scene at most one any-hit ray; no RNG state.
struct DirectDev {  // fields without a comment: the item source (device_item_source.hpp)
  const float4* surf;           // posW, N, diffuse, specular and prim are read
  const uint8_t* alive;
  float4* color;
  uint32_t* visible;            // query, optional: bit k = light k's term was added with s_k = 1
  uint32_t* traced;             // query, optional: bit k = a ray or a hint test was spent on light k
  const float4* gbPosition;
  const uint16_t* gbNormal;
  const uint16_t* gbDiffuse;
  const uint16_t* gbSpecRough;
  const uint32_t* pix;
  float4* out;
  QueryRange range;
};
// `cursor`: as launchTraceRays (the context's two words: zero when the launch starts, left zero)
void launchDirect(const SceneDev& S, const DirectDev& Q, bool gbuffer, bool hints, unsigned long long* cursor, LaunchGrids& G, int numCUs,
                  hipStream_t st);
// ris.hip: bdpt_ris_query (items are bdpt_surface records) and bdpt_ris_execute (items are the tile's pixels, read from the
// G-buffer).  Per alive item and sample `candidates` next-event candidates of the pass, one of them kept in a one-entry
// reservoir, and one any-hit ray for it (include/bdpt.h "Resampled direct lighting").
struct RisDev {  // fields without a comment: the item source (device_item_source.hpp)
  const float4* surf;           // posW, N, linearRoughness, diffuse and prim are read; GGX also V and specular
  const uint32_t* seeds;
  const uint8_t* alive;
  float4* color;
  uint32_t* seedsOut;           // query, optional: the state after 2 * candidates * samples draws (a dead item's: unchanged)
  uint32_t* traced;             // query, optional: the rays traversed per item (0 .. samples)
  uint4* reservoirs;            // optional: samples records per item, item-major (bdpt_ris_reservoir); execute: per frame pixel
  const float4* gbPosition;
  const uint16_t* gbNormal;
  const uint16_t* gbDiffuse;
  const uint16_t* gbSpecRough;  // GGX only: specular = rgb, rough = a * a
  const uint32_t* pix;
  float4* out;
  QueryRange range;             // minT: also of the occluder-hint test
  float camPos[3];              // execute, GGX: V = normalize(camPos - posW)
  float clampUpper;
  uint32_t candidates;          // 1 .. 32
  uint32_t samples;             // 1 .. 64
  uint32_t frameCount;          // execute
};
// A.n > 0: the AREA instances (the emitter table is light numLights while its W is positive).  `cursor`: as launchTraceRays
void launchRis(const SceneDev& S, const RisDev& Q, const AreaDev& A, bool gbuffer, bool ggx, bool hints, unsigned long long* cursor,
               LaunchGrids& G, int numCUs, hipStream_t st);
// reuse.hip: bdpt_reuse_query (items and pool entries are bdpt_surface records) and bdpt_reuse_execute (items are the
// tile's pixels, pool entries the pixels of a full-frame pool G-buffer).  Per alive item its own reservoir and those of up
// to eight pool entries are combined into one (the 1 / Z combination), and one any-hit ray is traced for the survivor
// (include/bdpt.h "Reservoir reuse").
struct ReuseDev {  // fields without a comment: the item source (device_item_source.hpp)
  const float4* surf;           // posW, N, linearRoughness, diffuse and prim are read; GGX also V and specular
  const uint32_t* seeds;
  const uint8_t* alive;
  float4* color;
  uint32_t* seedsOut;           // query, optional: the state after 1 + neighbors draws (a dead item's: unchanged)
  uint32_t* traced;             // query, optional: 1 where a ray was traversed
  const float4* gbPosition;
  const uint16_t* gbNormal;
  const uint16_t* gbDiffuse;
  const uint16_t* gbSpecRough;  // GGX only: specular = rgb, rough = a * a
  const uint32_t* pix;
  float4* out;
  const uint4* in;              // the items' own records (bdpt_reuse_reservoir): per item, execute: per frame pixel
  uint4* res;                   // optional: the combined records, indexed as `in`
  const float4* poolSurf;       // query: the pool's records, as `surf`,
  const uint8_t* poolAlive;     //   and optional alive bytes
  const float4* poolGbPosition; // execute: the pool's full-frame G-buffer, as the item's
  const uint16_t* poolGbNormal;
  const uint16_t* poolGbDiffuse;
  const uint16_t* poolGbSpecRough;
  const uint4* pool;            // the pool's reservoirs
  const uint32_t* neighborIndex;  // neighbors pool indices per item; execute, optional: per frame pixel
  QueryRange range;
  float camPos[3];              // execute, GGX: V = normalize(camPos - posW) of an item,
  float poolCamPos[3];          //   and of a pool pixel
  uint32_t poolNum;             // execute: width * height
  uint32_t neighbors;           // 0 .. 8
  uint32_t inM, poolM, maxM;    // candidate counts (0: the record's M word)
  float normalMin, planeMax;    // a neighbour's rejection tests
  float clampUpper;
  uint32_t frameCount;          // execute
  uint32_t width, height;       // execute: the frame
  uint32_t radius;              // execute without neighborIndex: 0 = slot 0 is the item's own pixel, else drawn offsets
};
// A.n > 0: the AREA instances.  `cursor`: as launchTraceRays
void launchReuse(const SceneDev& S, const ReuseDev& Q, const AreaDev& A, bool gbuffer, bool ggx, unsigned long long* cursor, LaunchGrids& G,
                 int numCUs, hipStream_t st);
void launchGather(const FrameDev& F, const PathBuf& P, const FrameVariant& V, uint32_t* lazyList, uint32_t* lazyCount, hipStream_t st);
void launchLazyGen(const FrameDev& F, const PathBuf& P, const uint32_t* list, const uint32_t* listCount, int batch, hipStream_t st);
void launchLazyCheck(const FrameDev& F, const PathBuf& P, const FrameVariant& V, const uint32_t* list, const uint32_t* listCount,
                     int batch, uint32_t* nextList, uint32_t* nextCount, hipStream_t st);
constexpr int kLazyBatchDiv = 8;    // a front round examines ceil(pairs / 8) candidates per pending pixel
constexpr int kMaxLazyRounds = 8;   // cursor blocks reserved for lazy rounds  // rounds per frame; batch = ceil(pairs / rounds)
// out[pix] = saturate(out[pix] + splat) for the tile's pixels.  tileLocal: `splat` holds the tile's accumulators in
// tile-local order (a reduce-scattered chunk); otherwise SplatLayout order, starting at frame row splatRow0 (owners == 1).
void launchResolve(const unsigned long long* splat, bool tileLocal, uint32_t splatRow0, const SplatLayout& L, float* out, uint32_t W,
                   const uint32_t* pix, uint32_t Np, hipStream_t st);
// the frame's own resolve: launchResolve for a plain frame (whole context, SplatLayout order), the group or masked one
void launchFrameResolve(const FrameDev& F, const PathBuf& P, const FrameVariant& V, hipStream_t st);
// bdpt_adaptive_update (adaptive.hip; exact arithmetic in include/bdpt.h "Adaptive sampling").  `scratch`: two words of
// the context, zero when the launch starts; the launch leaves them zero.
struct AdaptiveDev {
  float4* mean;
  float* m2;
  uint32_t* count;
  uint8_t* mask;
  uint32_t* active;
  float4* frame;
  uint32_t W, H;
  float threshold, epsilon;
  uint32_t minSamples, maxSamples, blockSize;
};
void launchAdaptiveUpdate(const AdaptiveDev& A, unsigned long long* scratch, hipStream_t st);
void launchAdaptiveReset(const AdaptiveDev& A, hipStream_t st);
void launchAccumulate(float* last, float* cur, uint32_t accumCount, uint32_t maxAccum, uint64_t numTexels, hipStream_t st);
void launchAccumulateTile(float* last, float* cur, uint32_t accumCount, uint32_t maxAccum, const uint32_t* pix, uint32_t Np,
                          hipStream_t st);
// rows of a tile <-> a contiguous run (bdpt_tile_pack / bdpt_tile_unpack): elements of 4, 8 or 16 bytes
void launchTilePack(const void* frame, void* packed, uint32_t bytesPerPixel, const uint32_t* pix, uint32_t Np, hipStream_t st);
void launchTileUnpack(const void* packed, void* frame, uint32_t bytesPerPixel, uint32_t W, uint32_t H, uint32_t stripeRows, uint32_t owners,
                      uint32_t owner, uint32_t packedRows, hipStream_t st);
void launchTestRng(const uint32_t* v0, const uint32_t* v1, uint32_t n, uint32_t draws, uint32_t* states, float* floats,
                   hipStream_t st);
void launchTestTrace(const SceneDev& S, const float* rays, uint32_t n, int mode, int32_t* prim, float* tuv, hipStream_t st);
void launchTestTraceShadow(const SceneDev& S, const float* planes, uint32_t cap, const uint32_t* count, uint32_t* head, uint8_t* vis,
                           DevCounters* counters, float tmin, int numCUs, hipStream_t st);
void launchTestBsdf(const float* in, uint32_t n, uint32_t matIndex, float* out, hipStream_t st);

// area_lights.hip: the emitter table of BDPT_PARAM_AREA_LIGHTS.
// Build (bdpt_prepare / first use; may synchronise): launchAreaMarkReferenced sets referenced[t] = 1 for every triangle a
// leaf of the tree references (only needed when the build dropped triangles; the refit plan names the leaves);
// launchAreaCount writes per-wave emitter counts of the triangles (referenced may be NULL: all referenced) and scans them
// into blockBase (exclusive) and counts[0..1] = emitters, textured emitters; launchAreaCompact then writes the emitters'
// primitives in ascending order.  Refresh (every bdpt_update_geometry; no allocation, no synchronisation):
// launchAreaRefresh recomputes weights and the CDF from the current shading records.  `blocks` holds one float and one
// word per 64 emitters (wavesFor(n)).
void launchAreaMarkReferenced(const BvhRefitNode* nodes, uint32_t numNodes, const uint4* recs, uint8_t* referenced, hipStream_t st);
void launchAreaCount(const SceneDev& S, uint32_t numTris, const uint8_t* referenced, uint32_t* blockCount, uint32_t* blockBase,
                     uint32_t* counts, hipStream_t st);
void launchAreaCompact(const SceneDev& S, uint32_t numTris, const uint8_t* referenced, const uint32_t* blockBase,
                       const uint32_t* alphaTris, uint32_t numAlphaTris, float4* emit, hipStream_t st);
void launchAreaRefresh(const SceneDev& S, const AreaDev& A, float* blockSum, uint32_t* blockLast, hipStream_t st);
// bdpt_test_area_light_sample: mode 0 light-subpath start, mode 1 NEE sample (16 floats per item out; include/bdpt.h)
void launchTestAreaSample(const SceneDev& S, const AreaDev& A, int mode, const uint32_t* states, const float* points, uint32_t n,
                          float* out, hipStream_t st);
// bdpt_test_alpha: one lane per (prim, u, v); variant 0 alphaTestFails, 1 and 2 the two slots of alphaTestFails2 (include/bdpt.h)
void launchTestAlpha(const SceneDev& S, const uint32_t* alphaTris, uint32_t numAlphaTris, uint32_t variant, const uint32_t* prim,
                     const float* uv, uint32_t n, uint8_t* out, hipStream_t st);

}  // namespace bdpt
