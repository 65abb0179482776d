/*
 * bdpt.h — C ABI of the MI355X-native bidirectional path-tracing render pass.
 *
 * This is the drop-in boundary.  Every entry point names the
 * reference interface it replaces (paths relative to /root/reference/src):
 *
 *   bdpt_create / bdpt_destroy      RayLaunch::create + compileRayProgram
 *                                   (SharedUtils/RayLaunch.h:85-101,
 *                                    BidirectionalPathtracing/Passes/BDPTPass.cpp:34-47)
 *   bdpt_set_scene                  RayLaunch::setScene -> RtProgramVars/RtScene::createTlas,
 *                                   RtModel::buildAccelerationStructure
 *                                   (SharedUtils/RayLaunch.cpp:105-167,
 *                                    Falcor/Framework/Source/Raytracing/RtModel.cpp:181-254,
 *                                    Falcor/Framework/Source/Raytracing/RtScene.cpp:220-308)
 *   bdpt_update_geometry / bdpt_set_lights / bdpt_get_refit_info
 *                                   RtScene::update marking the acceleration structure for refit every frame and
 *                                   RtScene::createTlas updating it with PERFORM_UPDATE
 *                                   (Falcor/Framework/Source/Raytracing/RtScene.cpp:74-83, 244-283): animated scenes
 *   bdpt_trace_rays                 TraceRay from a caller's own ray-generation shader
 *                                   (CommonPasses/Data/CommonPasses/aoTracing.rt.hlsl:112,
 *                                    lambertianPlusShadows.rt.hlsl:62, simpleDiffuseGI.rt.hlsl:127): ray queries
 *   bdpt_camera_rays / bdpt_shade_hits / bdpt_bsdf_query
 *                                   GBufferRayGen's camera, the hit shading (getVertexAttributes,
 *                                   simplePrepareShadingData) and sampleBRDF / evalBRDF for a caller's own
 *                                   integrator: surface queries
 *   bdpt_light_query                sampleLight (BDPT/BDPTUtils.hlsli:140-152) and the light part of a next-event term
 *                                   (getLightData, ggxDirect / lambertianDirect) for a caller's own integrator: light
 *                                   queries
 *   bdpt_connect_query              the vertex connections (BDPTMain.rt.hlsl:212-233, evalGWithoutV /
 *                                   getUnweightedContribution BDPTUtils.hlsli:172-224) and the light-tracing splat
 *                                   (BDPTMain.rt.hlsl:171-208, getLaunchIndexFromDirection BDPTUtils.hlsli:129-138)
 *                                   for a caller's own integrator: connection queries
 *   bdpt_splat_add                  the splat's write to the pixel it lands in (BDPTMain.rt.hlsl:186-204) as the
 *                                   fixed-point sum bdpt_splat_buffer describes below, for a caller's lists
 *   bdpt_walk_query                 shootRay and the walks' closest-hit and miss shaders (BDPTMain.rt.hlsl:106-145,
 *                                   BDPT/globalIlluminationRay.hlsli:1-45) for a caller's own integrator: walk queries
 *   bdpt_set_environment            the "EnvironmentMap" channel BDPTPass requests (BDPTPass.cpp:29; bound by no shader
 *                                   of the pass in the reference): read only with BDPT_PARAM_ENV_ON_MISS
 *   bdpt_bvh_build_check / _hash, bdpt_host_bvh_*
 *                                   (none in the reference: the DXR driver's acceleration structure is opaque) —
 *                                   host-only checks of the builder and a CPU walk of its tree for tests and tools
 *   bdpt_set_camera                 gCamera constant buffer (CameraData,
 *                                   Falcor/Framework/Source/Data/HostDeviceSharedCode.h:69-99;
 *                                   Camera::calculateCameraParameters, Graphics/Camera/Camera.cpp:129-136)
 *   bdpt_gbuffer_execute            LightProbeGBufferPass::execute -> DispatchRays of GBufferRayGen
 *                                   (CommonPasses/LightProbeGBufferPass.cpp:104-161,
 *                                    CommonPasses/Data/CommonPasses/lightProbeGBuffer.rt.hlsl:63-159)
 *   bdpt_execute                    BDPTPass::execute -> RayLaunch::execute -> DispatchRays of
 *                                   SimpleDiffuseGIRayGen (BidirectionalPathtracing/Passes/BDPTPass.cpp:70-107,
 *                                   SharedUtils/RayLaunch.cpp:200-223,
 *                                   BidirectionalPathtracing/Data/BDPTMain.rt.hlsl:42-234)
 *   bdpt_splat_buffer / bdpt_set_splat_buffer / bdpt_resolve
 *                                   the cross-pixel gOutput[id] read-modify-write of the
 *                                   light-tracing loop (BDPTMain.rt.hlsl:186-204), made
 *                                   deterministic: fixed-point atomics into a separate buffer,
 *                                   one final saturate
 *   bdpt_resize / bdpt_resize_stripes / bdpt_prepare
 *                                   RenderPass::resize + the lazy texture creation of
 *                                   ResourceManager::requestTextureResource (SharedUtils/RenderPass.h:42,
 *                                   SharedUtils/ResourceManager.cpp:210-241): per-tile path state; the striped form
 *                                   and bdpt_resolve_tile / bdpt_accumulate_tile / bdpt_get_tile_info have no
 *                                   counterpart (the reference renders on one GPU: a single DispatchRays,
 *                                   Falcor API/D3D12/D3D12RenderContext.cpp:350-384) — they are the multi-GPU
 *                                   tiling of SURVEY.md §8e
 *   bdpt_accumulate                 SimpleAccumulationPass::execute + accumulate.ps.hlsl
 *                                   (CommonPasses/SimpleAccumulationPass.cpp:104-134,
 *                                    CommonPasses/Data/CommonPasses/accumulate.ps.hlsl:28-42)
 *   bdpt_bmfr_execute / bdpt_bmfr_reset
 *                                   BlockwiseMultiOrderFeatureRegression::execute / resize
 *                                   (BidirectionalPathtracing/Passes/DenoisePass.cpp:146-279 with
 *                                    Data/preprocess.ps.hlsl:33-165, regressionCP.hlsl:100-500,
 *                                    postprocess.ps.hlsl:22-91); the pass is off by default
 *                                   (DenoisePass.h:71) and outside radiance parity
 *   bdpt_camera_view_proj           Camera::calculateCameraParameters' viewProjMat without jitter
 *                                   (Falcor Graphics/Camera/Camera.cpp:60-109), for prevViewProjMat
 *   BDPT_PARAM_AREA_LIGHTS / bdpt_get_area_light_info / bdpt_test_area_light_sample
 *                                   the TODO at the start of the light subpath ("Now assume point light source is used,
 *                                   but we can extend it to area and directional light", BidirectionalPathtracing/Data/
 *                                   BDPTMain.rt.hlsl:117-120): emissive triangles as one more light of sampleLight's
 *                                   uniform choice (BDPTUtils.hlsli:140-152), evaluated by ggxDirect / lambertianDirect
 *                                   (MaterialUtils.hlsli:149-184, 288-307) for next-event estimation
 *   bdpt_get_counters               (none in the reference; replaces nothing — ray tallies
 *                                    needed by the Mrays/s metric)
 *   bdpt_last_error                 Falcor logError / silent no-op conventions
 *                                   (BidirectionalPathtracing/Passes/BDPTPass.cpp:76)
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on
 * success and a negative BDPT_E_* code on failure; nothing throws across the
 * boundary; `stream` is a hipStream_t passed as void* (NULL = default stream).
 * All image buffers are device pointers, row-major, pitch = width.
 */
#ifndef BDPT_H_
#define BDPT_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BDPT_OK 0
#define BDPT_E_INVALID (-1)  /* bad argument */
#define BDPT_E_STATE (-2)    /* scene / camera / size not set */
#define BDPT_E_HIP (-3)      /* HIP runtime error, see bdpt_last_error */
#define BDPT_E_NOMEM (-4)
#define BDPT_E_LIMIT (-5)    /* exceeds a documented limit (lights, depth) */

#define BDPT_MAX_LIGHTS 16   /* MAX_LIGHT_SOURCES, Falcor Data/HostDeviceSharedMacros.h:152 */
#define BDPT_MAX_DEPTH 16    /* reference caps at 8 (BDPTPass.h:33); storage here is depth-parametric */

/* Light types, Falcor Data/HostDeviceSharedMacros.h:145-150 */
#define BDPT_LIGHT_POINT 0
#define BDPT_LIGHT_DIRECTIONAL 1

/* Material flag bit layout is Falcor's (Data/HostDeviceSharedMacros.h:69-123). */
#define BDPT_SHADING_MODEL_METAL_ROUGH 0u
#define BDPT_SHADING_MODEL_SPEC_GLOSS 2u
#define BDPT_CHANNEL_UNUSED 0u
#define BDPT_CHANNEL_CONST 1u
#define BDPT_CHANNEL_TEXTURE 2u
#define BDPT_NORMAL_MAP_UNUSED 0u
#define BDPT_NORMAL_MAP_RGB 1u
#define BDPT_NORMAL_MAP_RG 2u
#define BDPT_ALPHA_MODE_OPAQUE 0u
#define BDPT_ALPHA_MODE_MASK 1u
#define BDPT_FLAG_SHADING_MODEL(f) (((f) >> 0) & 7u)
#define BDPT_FLAG_DIFFUSE_TYPE(f) (((f) >> 3) & 7u)
#define BDPT_FLAG_SPECULAR_TYPE(f) (((f) >> 6) & 7u)
#define BDPT_FLAG_EMISSIVE_TYPE(f) (((f) >> 9) & 7u)
#define BDPT_FLAG_NORMAL_MAP_TYPE(f) (((f) >> 12) & 3u)
#define BDPT_FLAG_ALPHA_MODE(f) (((f) >> 17) & 3u)
#define BDPT_FLAG_DOUBLE_SIDED(f) (((f) >> 19) & 1u)
#define BDPT_MAKE_FLAGS(model, dif, spec, emis, nmap, alpha, dbl)                              \
  ((uint32_t)(((model) & 7u) | (((dif) & 7u) << 3) | (((spec) & 7u) << 6) | (((emis) & 7u) << 9) | \
              (((nmap) & 3u) << 12) | (((alpha) & 3u) << 17) | (((dbl) & 1u) << 19)))

/* MaterialData (Falcor Data/HostDeviceSharedCode.h:119-135) without the
 * resource handles; textures are indices into bdpt_scene_desc.textures. 64 B. */
typedef struct bdpt_material {
  float baseColor[4];
  float specular[4];
  float emissive[3];
  float alphaThreshold;
  float IoR;
  uint32_t flags;
  int16_t texBaseColor; /* -1 = none */
  int16_t texSpecular;
  int16_t texEmissive;
  int16_t texNormal;
} bdpt_material;

/* One mip-0 RGBA8 image.  The reference binds a linear/wrap sampler to every
 * scene texture (SharedUtils/SceneLoaderWrapper.cpp:65-68) and only samples
 * at explicit LOD 0 on this path (BDPTUtils.hlsli:6, lightProbeGBuffer.rt.hlsl:102). */
typedef struct bdpt_texture {
  const uint8_t* rgba8; /* host pointer, width*height*4 bytes, row 0 first */
  uint32_t width;
  uint32_t height;
  uint32_t srgb; /* 1: rgb channels are sRGB-encoded (Falcor default for colour textures) */
  uint32_t reserved;
} bdpt_texture;

/* The LightData fields this path reads (Falcor Data/HostDeviceSharedCode.h:199-217). 64 B. */
typedef struct bdpt_light {
  float posW[3];
  uint32_t type;
  float dirW[3];
  float openingAngle;
  float intensity[3];
  float cosOpeningAngle;
  float penumbraAngle;
  float reserved[3];
} bdpt_light;

/* World-space, instancing flattened (the reference loads with
 * Model::LoadFlags::RemoveInstancing, SharedUtils/SceneLoaderWrapper.cpp:58).
 * Every vertex stream has 12-byte stride, including texcoords (.xy used), as in
 * Falcor's ray-tracing vertex fetch (ShadingUtils/Raytracing.slang:79-85). */
typedef struct bdpt_scene_desc {
  uint32_t numVertices;
  uint32_t numTriangles;
  uint32_t numMaterials;
  uint32_t numTextures;
  uint32_t numLights;
  uint32_t reserved;
  const float* positions;
  const float* normals;
  const float* bitangents; /* may be NULL when no material has a normal map */
  const float* texcoords;  /* may be NULL when no material samples a texture */
  const uint32_t* indices;     /* 3 per triangle */
  const uint32_t* triMaterial; /* 1 per triangle */
  const bdpt_material* materials;
  const bdpt_texture* textures;
  const bdpt_light* lights;
} bdpt_scene_desc;

/* posW + cameraU/V/W of CameraData (Data/HostDeviceSharedCode.h:86-92). */
typedef struct bdpt_camera {
  float posW[3];
  float cameraU[3];
  float cameraV[3];
  float cameraW[3];
} bdpt_camera;

/* GlobalCB of BDPTMain.rt.hlsl:12-22 plus build-only switches. */
typedef struct bdpt_params {
  float minT;            /* gMinT, default 1e-4 (SharedUtils/ResourceManager.h:150) */
  uint32_t frameCount;   /* gFrameCount, starts at 0x1337 (BDPTPass.h:44) */
  uint32_t matIndex;     /* gMatIndex 0 = GGX, 1 = Lambertian */
  float refractiveIndex; /* gRefractiveIndex — read by no shader, kept for layout */
  uint32_t maxDepth;     /* gMaxDepth */
  float emitMult;        /* gEmitMult — read by no shader */
  float clampUpper;      /* gClampUpper, default 0.9; a number >= 0, see BDPT_MAX_CLAMP_UPPER_SPLAT */
  float pixelJitter[2];  /* gPixelJitter = kMSAA[(frame+1)%8]/16 + 0.5 */
  uint32_t flags;        /* BDPT_PARAM_* */
} bdpt_params;

/* clampUpper.  The reference clamps every term to [0, gClampUpper] (clampVec, MaterialUtils.hlsli:15-18) and its UI keeps the
 * bound in [0.001, 1] (BDPTPass.cpp:64).  Here light-tracing terms are summed in 2^-32 fixed point (quirk 6): a term c lands as (uint64_t)(c * 2^32),
 * which is defined for 0 <= c < 2^32 only (beyond it the host conversion and the device's differ, and neither saturates).
 * So every frame entry point (bdpt_execute, _tail, _masked, _light_groups, _grouped) refuses
 *   - a clampUpper that is NaN or negative: BDPT_E_INVALID (clampVec would return the bound itself for every term);
 *   - a clampUpper above BDPT_MAX_CLAMP_UPPER_SPLAT = 2^32 - 256, the largest float below 2^32, unless the frame has no
 *     light-tracing stage (BDPT_PARAM_NO_SPLAT): BDPT_E_LIMIT.  NEE and connection terms are float sums and take any bound,
 *     +inf included.
 * Within the limit the accumulators are exact sums modulo 2^64 in any order; they stay below 2^64, and so mean what they
 * say, while (splats landing on one pixel) * clampUpper < 2^32. */
#define BDPT_MAX_CLAMP_UPPER_SPLAT 4294967040.0f

#define BDPT_PARAM_COUNTERS 1u      /* also tally node / triangle visits (slower; not for timing).  Ray tallies are always on. */
#define BDPT_PARAM_DEFER_RESOLVE 2u /* leave splats in the splat buffer; caller runs bdpt_resolve */
#define BDPT_PARAM_NO_NEE 4u        /* partial images for stage-wise parity (SURVEY §8c iv) */
#define BDPT_PARAM_NO_SPLAT 8u
#define BDPT_PARAM_NO_CONNECT 16u
/* sampleGGXBRDF never writes its `out bool isSpecular` (MaterialUtils.hlsli:209-252): undefined in
 * HLSL.  Default build definition: false.  With this flag: true iff the GGX lobe was sampled. */
#define BDPT_PARAM_SPECULAR_FROM_LOBE 32u
/* Weight every strategy with getWeightPower / getWeightLinear (BDPTUtils.hlsli:226-278) instead of the
 * uniform 1/k the reference applies (it defines these functions but never calls them). */
#define BDPT_PARAM_MIS_POWER 64u
#define BDPT_PARAM_MIS_LINEAR 128u
/* Two-phase execute for tiled multi-GPU hosts: bdpt_execute returns once every launch that writes the
 * splat buffer is enqueued (walks, NEE, splats, non-zero connections); bdpt_execute_tail enqueues the rest
 * (zero-valued connection rounds, resolve unless deferred).  The host starts its splat exchange between
 * the two so it overlaps the tail.  Same image as the one-call form, bit for bit. */
#define BDPT_PARAM_DEFER_TAIL 256u
/* Do not zero the counters at the start of this execute: tallies add up over frames until an execute
 * without the flag (lets a host keep several frames in flight without a per-frame read-back;
 * raysPrimary in bdpt_get_counters stays one frame's worth). */
#define BDPT_PARAM_KEEP_COUNTERS 512u
/* Lighting the reference leaves out of its walks (RayMiss returns black, globalIlluminationRay.hlsli:14-19; emissive is
 * only added for the primary hit, BDPTMain.rt.hlsl:155-158).  Off by default = the
 * reference's image.  Build definitions, both for the EYE walk only and both weighted like the path-tracing strategy
 * of the same length (uniform 1/edges, as the reference weights its NEE terms), clamped with gClampUpper, added
 * without saturate after the pixel's own emissive term and before the NEE terms, in bounce order:
 *   ENV_ON_MISS    a ray leaving eye vertex k that misses adds cameraPath[k].color * environment(dir) / (k + 1); the
 *                  environment is the lat-long lookup of the G-buffer pass's miss shader
 *                  (lightProbeGBuffer.rt.hlsl:63-74) on the map given to bdpt_set_environment, else its constant colour
 *   EMISSIVE_HITS  a ray leaving eye vertex k that hits an emissive surface adds cameraPath[k].color * emissive / (k + 1) */
#define BDPT_PARAM_ENV_ON_MISS 1024u
#define BDPT_PARAM_EMISSIVE_HITS 2048u
/* Area lights: emissive triangles light the scene through next-event estimation and light subpaths (build definition;
 * off by default, and off every frame is the frame without it, bit for bit).
 *   Emitters: the triangles whose material's emissive channel is BDPT_CHANNEL_CONST with a Rec.709 luminance > 0 or
 *     BDPT_CHANNEL_TEXTURE, except those alpha clipping dropped (bdpt_bvh_info.numDropped), in ascending primitive order.
 *     Weight w = area * lambda: area = 0.5 |cross(p1 - p0, p2 - p0)| from the current positions (after
 *     bdpt_update_geometry, the updated ones); lambda = luminance of the emissive constant (CONST) or 1 (TEXTURE: the
 *     largest luminance a decoded RGBA8 texel has), so the pdf is positive wherever emission can be.  CDF = inclusive fp32
 *     prefix sums of the weights in this order: each wave of 64 emitters (emitters 64 j .. 64 j + 63, missing ones weigh
 *     +0) is scanned Hillis-Steele style (offsets 1, 2, 4, ..., 32: v[l] = v[l] + v[l - o] for l >= o); one wave then
 *     scans the wave sums (each scan's last value) the same way in chunks of 64 with a running carry (from 0): the prefix
 *     of wave j is carry for the chunk's first wave, else carry + the in-chunk inclusive value of wave j - 1, and after
 *     each chunk carry = carry + the chunk's last inclusive value; an emitter's CDF value is its wave's prefix + its
 *     in-wave value (wave 0: the in-wave value alone).  W = the last CDF value.  No emitter, or W == 0 (not > 0): the
 *     switch changes nothing, bit for bit.
 *   Selection: all emitters together are light numLights; the light count of the whole frame (the uniform choice of
 *     init_paths and of every NEE term, shadowMult, lightPath[0].pdf) is numLights + 1.  numLights >= 1 stays required.
 *   A point from uniforms (a, u1, u2): emitter i = the first whose CDF value is > a * W (none, by rounding: the last with
 *     w > 0); barycentrics b1 = u2 sqrt(u1), b2 = 1 - sqrt(u1) (the point is (1 - b1 - b2) p0 + b1 p1 + b2 p2); position
 *     and emission Le exactly as the hit shading gives them there (bdpt_shade_hits without the normal map, the same texture
 *     fetch: NEE and EMISSIVE_HITS read one emission).  Le = 0 where the material is alpha-masked and the alpha test fails
 *     at the point, or where the geometric normal n_g = normalize(cross(p1 - p0, p2 - p0)) has zero length.  Area pdf
 *     p_A = w_i / (W * area_i).  Emission is two-sided, as EMISSIVE_HITS and the G-buffer treat it.
 *   Draws (App. A of SURVEY.md, continued):
 *     light subpath start (item 5): after the selection draw picks numLights: a, u1, u2, the side s (n = s < 0.5 ? n_g :
 *       -n_g), then getCosHemisphereSample(seed, n) (two draws); lightPath[0].pos = x, .color = Le * 2 pi / p_A
 *       (Le |cos| / (p_A p_omega), not divided by the selection probability, as for point lights), .pdf = 1 / (numLights
 *       + 1); seedL = the state after these draws.
 *     NEE term t (item 8): its draw r (the (t+1)-th after seedL) is unchanged; when it picks numLights, a, u1, u2 come
 *       from initRand(<state after r>, 0x41524541u), so no other term's draws move.  L = (x - pos) / d; the light
 *       intensity ggxDirect / lambertianDirect take is Le |dot(n_g, L)| / (p_A d^2); the shadow ray has tmax = d (1 - 1e-4)
 *       (the emitter does not occlude its own sample) and no occluder hint.  A term with d^2 == 0 or a non-finite
 *       intensity is +0.
 *   Supported with whole-frame, band and stripes contexts, bdpt_execute_masked, DEFER_RESOLVE / DEFER_TAIL and
 *   EMISSIVE_HITS / ENV_ON_MISS.  BDPT_E_INVALID with BDPT_PARAM_MIS_POWER / _LINEAR (the pdf of an area-light vertex in
 *   the MIS prefix is a design question of its own) and with bdpt_execute_light_groups (its group planes have no slot for
 *   it: bdpt_execute_grouped assigns the table a group).  The table is made by bdpt_prepare(BDPT_PREPARE_AREA_LIGHTS) or
 *   by the first frame with the switch (which then must not be inside a stream capture: BDPT_E_STATE);
 *   bdpt_update_geometry refreshes its weights on its stream without allocating or synchronising. */
#define BDPT_PARAM_AREA_LIGHTS 4096u

/* RayGenCB of lightProbeGBuffer.rt.hlsl:45-52 + the miss shader's env map. */
typedef struct bdpt_gbuffer_params {
  float pixelJitter[2]; /* (0.5,0.5) when jitter is off */
  float lensRadius;
  float focalLen;
  uint32_t frameCount;  /* starts at 0xdeadbeef (CommonPasses/LightProbeGBufferPass.h:79) */
  uint32_t useThinLens;
  uint32_t envWidth;    /* gEnvMapRes */
  uint32_t envHeight;
  const float* envMap;  /* device RGBA32F, envWidth*envHeight*4 floats; NULL = constant envColor */
  float envColor[4];    /* default (0.5,0.5,0.8,1) (SharedUtils/ResourceManager.cpp:77-87) */
} bdpt_gbuffer_params;

/* The six G-buffer channels in the formats the first requester fixes
 * (CommonPasses/LightProbeGBufferPass.cpp:46-51): position RGBA32F, the rest
 * RGBA16F.  Device pointers, width*height texels each (full frame). */
typedef struct bdpt_gbuffer {
  float* worldPosition;          /* float4 */
  uint16_t* worldNormal;         /* half4: N.xyz, distance */
  uint16_t* materialDiffuse;     /* half4: diffuse.rgb, opacity | env colour on miss */
  uint16_t* materialSpecRough;   /* half4: specular.rgb, linearRoughness */
  uint16_t* materialExtraParams; /* half4: IoR, lightMap.rgb */
  uint16_t* emissive;            /* half4: emissive.rgb, 0 */
} bdpt_gbuffer;

/* Rows [y0,y1) of the full width×height frame are this context's tile.  The
 * light sub-path of every tile pixel still splats anywhere in the frame. */
typedef struct bdpt_tile {
  uint32_t y0;
  uint32_t y1;
} bdpt_tile;

/* Interleaved stripes for multi-GPU hosts: the frame's rows are dealt to numOwners contexts in
 * stripes of stripeRows rows; context `owner` renders stripes owner, owner + numOwners, ...  Cost that varies by
 * row (sky above, geometry below) then spreads over all owners, which contiguous bands do not give. */
typedef struct bdpt_stripes {
  uint32_t stripeRows;
  uint32_t numOwners;
  uint32_t owner;
} bdpt_stripes;

typedef struct bdpt_tile_info {
  uint32_t numRows;      /* rows this context renders */
  uint32_t numPixels;    /* numRows * width */
  uint32_t chunkRows;    /* rows of one owner's chunk of the splat buffer (its rows in order, zero-padded) */
  uint32_t numRowRanges; /* contiguous row runs (stripes) of this tile */
  uint64_t splatU64;     /* uint64 words of the whole splat buffer = numOwners * chunkU64 */
  uint64_t chunkU64;     /* uint64 words of one owner's chunk = chunkRows * width * 4 */
} bdpt_tile_info;

typedef struct bdpt_counters {
  uint64_t raysPrimary;
  uint64_t raysEyeExtend;
  uint64_t raysLightExtend;
  uint64_t raysNee;
  uint64_t raysSplat;
  uint64_t raysConnect;
  uint64_t nodeVisitsClosest; /* interior-node visits, closest-hit queries */
  uint64_t triTestsClosest;
  uint64_t nodeVisitsShadow;  /* interior-node visits, any-hit queries */
  uint64_t triTestsShadow;
  uint64_t pixelsValid;       /* G-buffer pixels with geometry */
  uint64_t splatsLanded;
  uint64_t raysConnectLazy;   /* subset of raysConnect traced by the gather stage for zero-valued pairs */
  uint64_t alphaTestsClosest; /* any-hit alpha tests (alphaTestFails, BDPTUtils.hlsli:115-127) run by closest-hit queries, */
  uint64_t alphaTestsShadow;  /* ... and by any-hit queries; with BDPT_PARAM_COUNTERS (the G-buffer ray is not tallied) */
  /* Any-hit queries answered "occluded" by their occluder hint — one triangle tried before the traversal: the nearest
   * triangle the light sees towards the vertex (next-event rays), the triangle the camera sees through the target pixel
   * (light-tracing rays).  Such a query never enters the ray queue and is NOT part of raysNee / raysSplat. */
  uint64_t hintedNee;
  uint64_t hintedSplat;
} bdpt_counters;

/* The environment secondary misses see (BDPT_PARAM_ENV_ON_MISS): an RGBA32F lat-long map (device pointer for
 * bdpt_set_environment, host pointer for the oracle) or, when envMap is NULL, a constant colour. */
typedef struct bdpt_environment {
  const float* envMap;
  uint32_t width, height;
  float color[4];
} bdpt_environment;

typedef struct bdpt_bvh_info {
  uint32_t numNodes;
  uint32_t numTriangles;
  uint32_t maxDepth;
  uint32_t nodeBytes; /* bytes per interior node */
  uint32_t triBytes;  /* bytes per leaf triangle */
  float sahCost;
  uint32_t maxStack;  /* worst-case traversal stack entries this tree needs (the device holds 32 per lane) */
  uint32_t reserved;
  uint32_t numReferences; /* leaf entries: a triangle cut by spatial pre-splitting has one per piece */
  uint32_t numDropped;    /* alpha-mode triangles without any reference: every texel they can sample fails the alpha test */
  uint32_t numAlphaMode;  /* triangles whose material is not AlphaModeOpaque (the reference runs the any-hit test on all of them) */
  uint32_t numAlwaysPass; /* of those: triangles whose texels all pass, traversed as opaque */
} bdpt_bvh_info;

typedef struct bdpt_ctx bdpt_ctx;

int bdpt_create(int device_ordinal, bdpt_ctx** out_ctx);
void bdpt_destroy(bdpt_ctx* ctx);
const char* bdpt_last_error(const bdpt_ctx* ctx);

/* Copies the scene and builds its acceleration structure on the context's device (what the reference leaves to the DXR
 * driver: Falcor RtModel.cpp:181-254, RtScene.cpp:220-308).  The caller keeps its arrays.  BDPT_E_INVALID for indices or
 * material ids out of range and for a triangle with a vertex position that is not finite or beyond 2^60 in magnitude
 * ("Animated scenes", Range); BDPT_E_NOMEM when host or
 * device memory runs out during the build; BDPT_E_LIMIT past 2^28 triangles / 2^31 records. */
int bdpt_set_scene(bdpt_ctx* ctx, const bdpt_scene_desc* scene);
int bdpt_get_bvh_info(const bdpt_ctx* ctx, bdpt_bvh_info* out);
int bdpt_set_camera(bdpt_ctx* ctx, const bdpt_camera* cam);
/* ResourceManager's "EnvironmentMap" channel as the BDPT pass would bind it (BDPTPass.cpp:29 requests it; no shader of
 * the pass reads it in the reference).  NULL = none (black).  Only read with BDPT_PARAM_ENV_ON_MISS, by bdpt_gi_query /
 * bdpt_gi_execute, and by the calls of "Environment lighting", whose sampling table (bdpt_env_prepare) this call drops: it
 * synchronises the device when there is one to drop. */
int bdpt_set_environment(bdpt_ctx* ctx, const bdpt_environment* env);

/* ---- Animated scenes: new vertex positions and lights between frames, without a rebuild ----
 * bdpt_update_geometry    RtScene::update marking the acceleration structure for refit every frame
 *                         (Falcor/Framework/Source/Raytracing/RtScene.cpp:74-83) and RtScene::createTlas updating it in
 *                         place with PERFORM_UPDATE (RtScene.cpp:244-283): the tree bdpt_set_scene built keeps its
 *                         topology, every box is refitted on the device (DESIGN.md "Refit").
 * bdpt_set_lights         the light data RtScene::update re-uploads when a light moves (RtScene.cpp:74-83 via
 *                         Scene::update); the light count stays.
 * bdpt_get_refit_info     (none in the reference: the DXR driver's structure is opaque) — what a caller needs to decide
 *                         when a rebuild (bdpt_set_scene) pays off.
 * bdpt_set_skin / bdpt_update_skinned
 *                         SkinningCache::update (Graphics/Model/SkinningCache.cpp, ComputeSkinning.cs.slang; attached in
 *                         RtScene.cpp:120) fed by Model::getBoneMatrices / getBoneInvTransposeMatrices: the vertices the
 *                         refit consumes are skinned on the device from a bone palette (below, "Skinning").
 * Topology, texture coordinates, materials, textures and the light count stay as the last bdpt_set_scene set them.
 * Both calls are enqueued on `stream`.  When the context's previous call used another stream, they first wait (an
 * event) for what that call enqueued, which ends with everything of the context's own second stream; bdpt_gbuffer_execute
 * and bdpt_execute calls enqueued after them on the same stream see the new scene.  Work on further streams is ordered by
 * the caller, as for the other calls of this interface.
 * Host inputs (BDPT_MEMORY_HOST) are checked and copied before the call returns: a position that is not finite, or
 * beyond 2^60 (below, "Range"), gives BDPT_E_INVALID and leaves the scene as it was.  Device inputs (BDPT_MEMORY_DEVICE) must stay valid until the stream
 * reaches the update, and their finiteness is the caller's responsibility.
 * After the first update, or after bdpt_prepare(BDPT_PREPARE_REFIT), a device-pointer update neither allocates nor
 * synchronises, so it can be captured into a hipGraph.
 * Errors: no scene BDPT_E_STATE; numVertices or the light count not the scene's BDPT_E_INVALID; more than
 * BDPT_MAX_LIGHTS lights BDPT_E_LIMIT.
 *
 * Piece-tight refit (opt-in, per context): bdpt_prepare(BDPT_PREPARE_REFIT_PIECES).  The plain refit bounds every
 * reference by its whole triangle, which gives away what spatial pre-splitting and alpha clipping bought at build time.
 * A reference stands for a piece of its triangle, and a per-vertex update maps a triangle affinely, so the piece keeps
 * its footprint in the triangle's barycentric plane.  The prepare derives, once, from the tree as built, a small
 * barycentric region per reference that contains its piece (DESIGN.md "Refit"); from then on every bdpt_update_geometry
 * and bdpt_update_skinned of the context bounds a reference by that region under the moved corners.  It implies
 * BDPT_PREPARE_REFIT, needs a scene and no update since bdpt_set_scene (after one the built boxes are gone), allocates
 * (24 bytes per record of the tree) and synchronises: BDPT_E_STATE without a scene, after an update, or inside a stream
 * capture.  bdpt_set_scene drops it.  Updates still neither allocate nor synchronise with device pointers and stay
 * capturable; bdpt_get_refit_info reports the tighter tree's cost.  Guarantees:
 *   - every query answers exactly as it does on a tree built at the new positions: images are bit-identical, as for the
 *     plain refit;
 *   - the records are a pure function of the built tree and the current positions;
 *   - a tree without split or clipped references gets exactly the plain refit's records.
 *
 * What poses an update may bring (bones that scale an axis to zero or mirror, morphs that close a mesh, a world whose
 * origin is not the model's), and the rules that make "exactly as on a tree built at the new positions" — and, for the
 * host tests, "exactly as a linear scan over the posed triangles" — hold for them, plain and by pieces:
 *   - Range.  Every |coordinate| <= 2^60 (1.15e18): up to there no box extent, squared diagonal or box area overflows, and
 *     bdpt_get_refit_info stays finite.  bdpt_set_scene and host-memory updates answer BDPT_E_INVALID beyond it, as for a
 *     position that is not finite.  Device-memory updates are not inspected: beyond the range the pad overflows and every
 *     box is NaN; no address in the tree derives from a position, so queries then miss, nothing else.
 *   - Far from the origin.  Every box is padded by the larger of 2e-5 of the scene's diagonal and 2^-21 of its largest
 *     |coordinate| (four ulps): the roundings that happen at the size of the coordinates (the padded planes, the
 *     quantiser's outward check, the corners of a piece box) add up to two ulps.  The second term counts from 42
 *     diagonals away from the origin; nearer, every record keeps the bits of the first alone.  At 1e7 extents the whole
 *     scene is a few fp32 values and nothing can be hit.
 *   - What the fp32 ray / triangle test itself cannot see is seen by nobody: scaled by 1e13 a scene keeps a few of its
 *     hits (products of three edge-sized factors overflow), from 1e15 on none, and none below 1e-20.
 *   - Zero direction components are exact in scenes no wider than 2^35 (3.4e10): the slab test multiplies a node's scale
 *     by the clamped reciprocal 1e30, which overflows for a node wider than 6.8e10; such rays may miss there.
 *   - Ill-conditioned hits (a documented limit).  With c = |e1 . (d x e2)| / (|e1| |e2| |d|), the (u, v) of a hit carry
 *     an error of about 4 eps / c of an edge.  Below c = 2^-6 — a needle (edges parallel up to rounding: the determinant
 *     is rounding noise, not zero), a sliver, or a ray inside a triangle's plane — the point a linear scan reports can lie
 *     outside the padded box of the triangle it reports, and a tree, built or refitted, may answer with another triangle
 *     or a miss.  Which of these a walk gives depends on the order in which it shrinks its interval, so on such a ray two
 *     walks of the same records — the device's kernels and the host hook's walk — may differ from one another too (one
 *     ray of 4096 on the courtyard's oblique plane does).  tests/edge_poses.py states the criterion in float64 and the tests count the rays it excuses (a
 *     flattened scene: 1.6 % of the closest hits).  Storing e1 = e2 = 0 for needles (sine of the corner below
 *     8 eps) ends these on flattened poses, but changes the records of every scene that holds a needle — the atrium has
 *     34, the tips of its cone caps — so it waits for a change that may move those hashes (DESIGN.md "Refit"). */
#define BDPT_MEMORY_HOST 0u
#define BDPT_MEMORY_DEVICE 1u
typedef struct bdpt_geometry_update {
  const float* positions;  /* numVertices x 3, required */
  const float* normals;    /* numVertices x 3; NULL = unchanged */
  const float* bitangents; /* numVertices x 3; NULL = unchanged (only for a scene that has them) */
  uint32_t numVertices;    /* must equal the scene's */
  uint32_t memory;         /* BDPT_MEMORY_HOST / BDPT_MEMORY_DEVICE */
  uint32_t flags;          /* BDPT_UPDATE_* */
  uint32_t reserved;
} bdpt_geometry_update;
/* do not re-trace the occluder cube maps (stale hints: the same image, fewer queries answered by a hint) */
#define BDPT_UPDATE_KEEP_LIGHT_MAPS 1u
typedef struct bdpt_refit_info {
  float sahCost;       /* SAH cost of the tree as it stands now (after the last update) */
  float sahCostBuilt;  /* the same formula for the tree bdpt_set_scene built (== bdpt_bvh_info.sahCost) */
  uint32_t numUpdates; /* updates since bdpt_set_scene */
  uint32_t reserved;
} bdpt_refit_info;
int bdpt_update_geometry(bdpt_ctx* ctx, const bdpt_geometry_update* upd, void* stream);
int bdpt_set_lights(bdpt_ctx* ctx, const bdpt_light* lights, uint32_t numLights, void* stream);
int bdpt_get_refit_info(bdpt_ctx* ctx, bdpt_refit_info* out); /* synchronises */

/* ---- Skinning: a bone palette per frame instead of three vertex streams ----
 * bdpt_set_skin gives the context the rest pose, four bone ids and four weights per vertex; bdpt_update_skinned then
 * takes the frame's bone matrices (a few KB), skins every vertex on the device into the context's own skinned streams
 * and does what bdpt_update_geometry does with them: the refit, the area-light table's refresh when there is a table, the
 * bitangent copy, the light maps' re-trace unless BDPT_UPDATE_KEEP_LIGHT_MAPS.  Ordering is bdpt_update_geometry's.
 *
 * Arithmetic: fp32, no contraction, exactly in this order (getBlendedBoneMat, mul(float4(pos, 1), boneMat),
 * mul(normal, invTransposeBoneMat) and mul(bitangent, (float3x3)boneMat) of the shader).  A matrix is 16 floats m[4r+c]:
 * the memory of the glm::mat4 getBoneMatrices hands over, translation in floats 12..14.  With the ids i0..i3 and the
 * weights w0..w3 of a vertex, M the `bones` and the rest position p, normal n, bitangent b:
 *   B[e]    = ((M[i0][e]*w0 + M[i1][e]*w1) + M[i2][e]*w2) + M[i3][e]*w3        T[e]: the same sum over `normalBones`
 *   pos'[c] = ((p.x*B[c] + p.y*B[4+c]) + p.z*B[8+c]) + B[12+c]
 *   n'[c]   = (n.x*T[c] + n.y*T[4+c]) + n.z*T[8+c]                             (not normalised, as in the shader)
 *   b'[c]   = (b.x*B[c] + b.y*B[4+c]) + b.z*B[8+c]
 * A vertex whose four weights are all zero (either sign) is static: its outputs are its rest values bit for bit, and its
 * ids are neither checked nor read (the flattened static part of a scene).  Weights are not renormalised.  The previous
 * frame's positions (gSkinnedPrevPositions, for motion vectors) are kept by bdpt_keep_pose ("Motion", after the surface queries), for every
 * kind of update, not by the skinning kernel.
 *
 * bdpt_set_skin synchronises and allocates everything a skinned update needs (rest streams, weights, ids, the skinned
 * streams, the device palette, and the refit plan as bdpt_prepare(BDPT_PREPARE_REFIT) does); not inside a stream capture
 * (BDPT_E_STATE).  After it a BDPT_MEMORY_DEVICE bdpt_update_skinned neither allocates nor synchronises and can be
 * captured into a hipGraph; its palettes must stay valid until the stream reaches the update, and their finiteness is the
 * caller's responsibility.  BDPT_MEMORY_HOST palettes are checked for finiteness and staged before the call returns;
 * inside a capture they give BDPT_E_STATE.  bdpt_update_geometry stays usable on a skinned context: it overwrites the
 * pose and leaves the rest pose alone.  A NULL desc drops the skin; bdpt_set_scene drops it too.
 * Errors (nothing is enqueued, the scene and the skin stay as they were): no scene, or bdpt_update_skinned /
 * bdpt_skinned_buffers without a skin BDPT_E_STATE; a NULL argument, numVertices or numBones not matching, numBones of 0,
 * a non-zero reserved, unknown flags or memory, bitangents for a scene without any, normalBones missing when the skin has
 * normals, a rest position, a weight or a host bone element that is not finite, an id >= numBones on a non-static vertex
 * BDPT_E_INVALID; numBones above BDPT_MAX_BONES BDPT_E_LIMIT. */
#define BDPT_MAX_BONES 1024
typedef struct bdpt_skin_desc { /* all HOST pointers, copied before the call returns */
  uint32_t numVertices;         /* must equal the scene's */
  uint32_t numBones;            /* 1 .. BDPT_MAX_BONES */
  const float* positions;       /* rest pose, numVertices x 3, required, finite */
  const float* normals;         /* rest pose; NULL = a skinned update leaves normals alone */
  const float* bitangents;      /* rest pose; NULL = left alone; only for a scene that has them */
  const float* boneWeights;     /* numVertices x 4 */
  const uint16_t* boneIds;      /* numVertices x 4 */
  uint32_t reserved[2];         /* 0 */
} bdpt_skin_desc;
int bdpt_set_skin(bdpt_ctx* ctx, const bdpt_skin_desc* desc);
typedef struct bdpt_skin_update {
  const float* bones;       /* numBones x 16 floats */
  const float* normalBones; /* numBones x 16: the inverse transposes; required iff the skin has normals */
  uint32_t numBones;        /* must equal the skin's */
  uint32_t memory;          /* BDPT_MEMORY_HOST / BDPT_MEMORY_DEVICE */
  uint32_t flags;           /* BDPT_UPDATE_KEEP_LIGHT_MAPS or 0 */
  uint32_t reserved;        /* 0 */
} bdpt_skin_update;
int bdpt_update_skinned(bdpt_ctx* ctx, const bdpt_skin_update* upd, void* stream);
/* device pointers of the context's skinned streams (NULL for a stream the skin lacks); valid until bdpt_set_skin /
 * bdpt_set_scene.  They hold the pose of the last bdpt_update_skinned once its stream has reached it. */
int bdpt_skinned_buffers(bdpt_ctx* ctx, const float** positions, const float** normals, const float** bitangents);
/* host-only, no context: the same arithmetic on the CPU, the same code as the kernel's (tests, callers that want the
 * pose on the host).  outNormals / outBitangents are required iff the desc has the stream; normalBones iff it has normals.
 * BDPT_E_INVALID / BDPT_E_LIMIT as above (the checks of the desc, NULL arguments, ids); the palettes' finiteness is not
 * checked. */
int bdpt_host_skin(const bdpt_skin_desc* desc, const float* bones, const float* normalBones, float* outPositions, float* outNormals,
                   float* outBitangents);

/* ---- Morph targets: blend-shape weights ahead of skinning and the refit ----
 * bdpt_set_morph gives the context per-target sparse vertex deltas; bdpt_update_morphed then takes the frame's weights
 * (one float per target) and, for a context with a skin, the frame's bone palettes, forms every vertex's morphed values,
 * skins them in the same registers where there is a skin, and does what bdpt_update_geometry does with the result: the
 * refit, the area-light table's refresh, the bitangent copy, the light maps' re-trace unless
 * BDPT_UPDATE_KEEP_LIGHT_MAPS.  Ordering is bdpt_update_geometry's.  The order of set-up calls is scene, skin, morph:
 * bdpt_set_skin (a NULL desc included) and bdpt_set_scene drop the morph.
 *
 * Base pose.  With a skin the base is the skin's rest pose: positions, normals and bitangents of the desc must be NULL,
 * and dNormals / dBitangents are allowed only for streams the skin has.  Without a skin `positions` is required;
 * normals / bitangents are optional, NULL meaning that an update leaves that stream alone, as bdpt_update_geometry
 * does, and the matching delta array must then be NULL too.
 *
 * Arithmetic: fp32, no contraction, exactly in this order.  For vertex v, every morphed stream and every component c:
 *   x = base[v][c]
 *   for every target t in ascending order that has an entry e for v and whose weight is not zero (either sign):
 *     x = x + weights[t] * d[e][c]                    (one rounding for the product, one for the sum)
 * A zero weight skips the term by definition (x + 0*d would turn a -0.0 into +0.0), so a vertex without entries, or
 * with only zero-weight entries, keeps its base bits exactly.  With a skin the morphed position / normal / bitangent
 * then take the place of the rest values in the skinning arithmetic above, which is unchanged; a static vertex (all four
 * bone weights zero) outputs its morphed values.  Nothing is renormalised.  Hence with a skin and all weights zero
 * bdpt_update_morphed leaves exactly the streams and records bdpt_update_skinned leaves for the same palettes.
 *
 * bdpt_set_morph synchronises and allocates everything a morphed update needs (the vertex-major copy of the entries,
 * the device weights, without a skin the base and the morphed streams, which hold the base until the first update, and
 * the refit plan); not inside a stream capture (BDPT_E_STATE).  After it a BDPT_MEMORY_DEVICE bdpt_update_morphed
 * neither allocates nor synchronises and can be captured into a hipGraph; weights and palettes must stay valid until the
 * stream reaches the update, and their finiteness is the caller's responsibility.  BDPT_MEMORY_HOST weights and palettes
 * are checked for finiteness and staged before the call returns; inside a capture they give BDPT_E_STATE.
 * bdpt_update_skinned and bdpt_update_geometry stay usable and unchanged on a context that has a morph; the former
 * ignores the morph.  With a skin the outputs are the skin's own skinned streams, so bdpt_skinned_buffers and
 * bdpt_morphed_buffers agree.
 * Errors (nothing is enqueued; scene, skin and morph stay as they were): no scene, bdpt_update_morphed /
 * bdpt_morphed_buffers without a morph, bdpt_set_morph inside a capture BDPT_E_STATE; a NULL argument, numVertices /
 * numTargets / numBones not matching, numTargets of 0, a non-zero reserved, unknown flags or memory, targetStart[0] != 0
 * or targetStart decreasing, a vertex id >= numVertices or ids not strictly ascending within a target, a delta, base value
 * or host weight (or host bone element) that is not finite, base pointers given with a skin or positions missing without
 * one, deltas for a stream the base lacks, bitangents for a scene without any, palettes missing with a skin or given
 * without one BDPT_E_INVALID; numTargets above BDPT_MAX_MORPH_TARGETS, 2^31 entries or more BDPT_E_LIMIT. */
#define BDPT_MAX_MORPH_TARGETS 1024
typedef struct bdpt_morph_desc { /* all HOST pointers, copied before the call returns */
  uint32_t numVertices;          /* must equal the scene's */
  uint32_t numTargets;           /* 1 .. BDPT_MAX_MORPH_TARGETS */
  const uint32_t* targetStart;   /* numTargets + 1, non-decreasing, [0] = 0: target t owns entries [targetStart[t], targetStart[t+1]) */
  const uint32_t* vertex;        /* per entry: vertex id, strictly ascending inside a target */
  const float* dPositions;       /* per entry x 3, required, finite */
  const float* dNormals;         /* per entry x 3, or NULL: normals are not morphed */
  const float* dBitangents;      /* per entry x 3, or NULL; only for a scene that has bitangents */
  const float* positions;        /* base pose, numVertices x 3: required without a skin, NULL with one */
  const float* normals;          /* base pose or NULL */
  const float* bitangents;       /* base pose or NULL */
  uint32_t reserved[2];          /* 0 */
} bdpt_morph_desc;
int bdpt_set_morph(bdpt_ctx* ctx, const bdpt_morph_desc* desc); /* NULL desc drops the morph */
typedef struct bdpt_morph_update {
  const float* weights;     /* numTargets */
  const float* bones;       /* required iff the context has a skin, else NULL: as bdpt_skin_update */
  const float* normalBones; /* required iff that skin has normals, else NULL */
  uint32_t numTargets;      /* must equal the morph's */
  uint32_t numBones;        /* must equal the skin's; 0 without a skin */
  uint32_t memory;          /* BDPT_MEMORY_HOST / BDPT_MEMORY_DEVICE, of weights and palettes alike */
  uint32_t flags;           /* BDPT_UPDATE_KEEP_LIGHT_MAPS or 0 */
  uint32_t reserved[2];     /* 0 */
} bdpt_morph_update;
int bdpt_update_morphed(bdpt_ctx* ctx, const bdpt_morph_update* upd, void* stream);
/* device pointers of the streams a morphed update writes (with a skin: the skinned streams; NULL for a stream the base
 * lacks); valid until bdpt_set_morph / bdpt_set_skin / bdpt_set_scene. */
int bdpt_morphed_buffers(bdpt_ctx* ctx, const float** positions, const float** normals, const float** bitangents);
/* host-only, no context: the same arithmetic on the CPU, the same code as the kernel's.  `skin`: the skin whose rest pose
 * is the base (the desc's base pointers NULL, bones required, normalBones iff it has normals), or NULL (the desc's own
 * base; bones and normalBones NULL).  outNormals / outBitangents are required iff the base has the stream.  The same desc
 * checks and codes as above; weights are checked for finiteness, palettes are not. */
int bdpt_host_morph(const bdpt_morph_desc* desc, const bdpt_skin_desc* skin, const float* weights, const float* bones,
                    const float* normalBones, float* outPositions, float* outNormals, float* outBitangents);

/* ---- Ray queries: a caller's own rays against the scene ----
 * bdpt_trace_rays         TraceRay from a caller's own ray-generation shader: ambient occlusion
 *                         (CommonPasses/Data/CommonPasses/aoTracing.rt.hlsl:112), shadow rays
 *                         (lambertianPlusShadows.rt.hlsl:62, BDPT/standardShadowRay.hlsli:40), one-bounce GI
 *                         (simpleDiffuseGI.rt.hlsl:127) — for picking, collision probes and custom integrators beside
 *                         the BDPT pass.  One call traces a batch of rays in device memory (DESIGN.md "Ray queries").
 * Semantics (those of the pass's own queries):
 *   - a ray hits a triangle at t when tmin < t < tmax; directions need not be unit length (t is in units of |dir|);
 *   - closest-hit ties go to the lowest primitive index; `prim` is the caller's input triangle index (also for the
 *     pre-split references of a large scene);
 *   - alpha-masked materials run the any-hit alpha test; triangles the build dropped as never visible are never hit;
 *   - a miss writes prim = -1 and t = u = v = 0; a ray with a NaN or zero direction, a NaN origin or tmax <= tmin misses;
 *   - with numRaysDevice set, rays at or beyond min(*numRaysDevice, numRays) are neither read nor written.
 * Ray contract (what a caller may send; DESIGN.md "Ray queries" has the measurements):
 *   - signed zeros in a direction are equivalent: (-0, -1, -0), the ray along -N of an axis-aligned wall, finds what
 *     (0, -1, 0) finds;
 *   - a direction component of magnitude below 1e-30 is treated as zero by the tree walk (its reciprocal is clamped to
 *     +-1e30): scale such directions up, and tmin / tmax down, before the call;
 *   - the answers are those of a linear scan over all triangles (hit on a shared vertex or edge, t == tmax, t == tmin,
 *     tmax = inf and negative tmin included) while the build's pad, 2e-5 of the scene's diagonal, exceeds an ulp of the
 *     coordinates: a scene nearer to the origin than some 300 of its diagonals.  Farther out a ray that grazes a
 *     triangle's vertex or edge can miss it: move the scene (and the rays) to the origin first.
 * Ordering: the call is enqueued on `stream`.  When the context's previous call used another stream, it first waits (an
 * event) for what that call enqueued, as bdpt_update_geometry does; it sees the scene as of the last update enqueued
 * before it.  Later calls of the context on the same stream are ordered behind it; work on further streams is ordered by
 * the caller, as for the other calls of this interface.  The inputs must stay valid, and the outputs are written, when the
 * stream reaches the call.
 * It neither allocates nor synchronises (no prepare step), so it can be captured into a hipGraph, and it changes nothing
 * bdpt_get_counters or bdpt_get_stage_times report.
 * INVARIANT: the persistent traversal kernels of one context share its stack-overflow area, so no two of them may be
 * resident at once.  This call keeps that by enqueuing only on `stream`, behind the context's previous call; a caller
 * who then renders on another stream orders that stream behind this one (an event), as for every call of the context.
 * Errors (nothing is enqueued): no scene BDPT_E_STATE; a NULL context or desc, an unknown mode, a missing or misaligned
 * buffer BDPT_E_INVALID.  numRays == 0 returns BDPT_OK and does nothing. */
typedef struct bdpt_ray {
  float org[3];
  float tmin;
  float dir[3];
  float tmax;
} bdpt_ray; /* 32 bytes */
typedef struct bdpt_hit {
  float t, u, v; /* barycentrics: the hit point is (1-u-v) v0 + u v1 + v v2 */
  int32_t prim;  /* input triangle index, -1 = miss */
} bdpt_hit;      /* 16 bytes */
#define BDPT_TRACE_CLOSEST 0u           /* closest hit */
#define BDPT_TRACE_CLOSEST_CULL_BACK 1u /* closest hit, RAY_FLAG_CULL_BACK_FACING_TRIANGLES (double-sided materials are kept) */
#define BDPT_TRACE_ANY 2u               /* RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH: visibility only */
typedef struct bdpt_trace_desc {
  const bdpt_ray* rays;          /* device, 16-byte aligned, numRays records */
  uint32_t numRays;              /* rays to trace; the capacity when numRaysDevice is set */
  uint32_t mode;                 /* BDPT_TRACE_* */
  const uint32_t* numRaysDevice; /* optional device word, read by the kernel: trace min(*numRaysDevice, numRays) rays */
  bdpt_hit* hits;                /* closest-hit modes: device, 16-byte aligned, one per ray (ignored for BDPT_TRACE_ANY) */
  uint8_t* visible;              /* BDPT_TRACE_ANY: device, one byte per ray, 1 = unoccluded (ignored otherwise) */
} bdpt_trace_desc;
int bdpt_trace_rays(bdpt_ctx* ctx, const bdpt_trace_desc* desc, void* stream);

/* ---- Surface queries: what the pass computes at a hit, for a caller's own integrator ----
 * bdpt_camera_rays        GBufferRayGen's primary rays (CP lightProbeGBuffer.rt.hlsl:110-135)
 * bdpt_shade_hits         getVertexAttributes + simplePrepareShadingData (+ applyNormalMap) at a hit: what the G-buffer
 *                         pass and the walk shade (Falcor ShadingUtils/Raytracing.slang:60-106, BDPT/BDPTUtils.hlsli:2-52)
 * bdpt_bsdf_query         sampleBRDF / evalBRDF (BDPT/MaterialUtils.hlsli:105-141, 186-329) on shaded records
 * With bdpt_trace_rays a caller runs camera rays -> trace -> shade -> sample -> trace on the device with the pass's own
 * arithmetic: each call runs the device function the pass runs, bit for bit (DESIGN.md "Surface queries").
 * Ordering, capture and counters: as bdpt_trace_rays — enqueued on `stream` behind the context's previous call; no
 * allocation and no synchronise (one kernel node in a captured graph); bdpt_get_counters and bdpt_get_stage_times are left
 * alone.  The shading calls see the scene as of the last bdpt_update_geometry enqueued before them.  num == 0 returns
 * BDPT_OK and does nothing.  Errors are found before anything is enqueued: no camera (bdpt_camera_rays) or no scene
 * (bdpt_shade_hits, bdpt_bsdf_query) BDPT_E_STATE; a NULL context or desc, a missing or misaligned buffer, unknown flags
 * or mode, matIndex > 1, a width or height of 0 or width * height >= 2^32 BDPT_E_INVALID.
 *
 * bdpt_camera_rays: the G-buffer pass's primary ray of every pixel of a width x height frame, in frame order
 * (rays[x + y * width]): pinhole, or thin lens with p->useThinLens, pixelJitter and frameCount as in p (the env fields are
 * ignored); tmin 0, tmax 1e38.  Always the whole frame (the context's size, tile and stripes play no part). */
int bdpt_camera_rays(bdpt_ctx* ctx, const bdpt_gbuffer_params* p, uint32_t width, uint32_t height, bdpt_ray* rays, void* stream);

/* bdpt_shade_hits: one record per hit.  hits[i] is shaded as seen from rays[i]'s origin (only the origin is read): the
 * interpolated position and normal, the textured material and, with BDPT_SHADE_NORMAL_MAP, the normal map — the
 * G-buffer pass's primary-hit shading (shadeHit<true>); without it the walk's (shadeHit<false>).  The ray origin takes the
 * place of the camera position, as the walk passes WorldRayOrigin(): with pinhole camera rays the records equal the
 * G-buffer channels before their half rounding.  The BSDF's roughness is linearRoughness * linearRoughness.  A miss
 * (prim < 0), or a prim that is not a triangle of the scene, writes prim -1, material 0xffffffff and every float 0.  With
 * numHitsDevice set, hits at or beyond min(*numHitsDevice, numHits) are neither read nor written.
 * Hit contract (tests/edge_surfaces.py has the families, DESIGN.md "Edge-case surfaces" the measurements): prim decides
 * every address; u and v may be anything a float holds — on a corner or an edge, outside the triangle, NaN or infinite —
 * and the record is that of the fp32 arithmetic as written, bit for bit the CPU oracle's.  The scene's texcoords need not
 * be finite either (bdpt_set_scene checks positions only; an infinite or NaN texcoord makes every UV of its triangle but
 * the one at its own corner NaN).
 *   Texture addressing: a sample at (u, v) of a w x h texture blends the texels around x = u * w - 0.5, y = v * h - 0.5:
 *     (int)floorf(x) and its successor under wrap addressing, fraction x - floorf(x), likewise in y.  The float -> int
 *     conversion is the hardware's (v_cvt_i32_f32): exact inside the int range, INT_MAX at and above 2^31, INT_MIN at and
 *     below -2^31, 0 for NaN; the oracle and every host restatement (csrc/texture_planes.h texelFloorInt) convert the same
 *     way.  So a texel index is inside the texture whatever the coordinate.  From |x| = 2^23 on the fraction is 0; an
 *     infinite or NaN x makes the fraction, and with it every texture-derived field, NaN (linearRoughness then is 0.08:
 *     maxf(0.08, NaN)).  The any-hit alpha test samples the same way; a NaN alpha is not below any threshold: it passes.
 *   Channel types: the type fields of bdpt_material::flags are 3 bits wide (the normal map's 2).  Every diffuse, specular or
 *     emissive type other than UNUSED (0) and CONST (1) samples the channel's texture at the hit's UV when the texture id is
 *     >= 0 and takes the constant factor when it is -1 (the rule of sampleTexture); the alpha test follows the same rule.
 *     Every shading model other than METAL_ROUGH decodes as SPEC_GLOSS; every normal-map type other than UNUSED and RGB as RG.
 *   Degenerate frames: an interpolated normal of length 0 (or one whose squared length under- or overflows fp32) gives a NaN
 *     N; an origin at posW a NaN V; dot(N, V) == 0 flips the normal of a double-sided material (the test is <=); a NaN
 *     dot(N, V) does not.  With BDPT_SHADE_NORMAL_MAP a bitangent parallel to N, or of length 0, gives a NaN N; a map texel
 *     whose decoded normal is 0 likewise.  A scene without bitangents, or a material whose texNormal is -1, is shaded
 *     without the map whatever its map type. */
typedef struct bdpt_surface {
  float posW[3];
  float dist;             /* length(posW - ray origin) */
  float N[3];             /* shading normal, flipped toward the origin for double-sided materials */
  float linearRoughness;
  float V[3];             /* normalize(ray origin - posW) */
  float IoR;
  float diffuse[3];
  float opacity;
  float specular[3];
  uint32_t material;      /* material index, 0xffffffff on a miss */
  float emissive[3];
  int32_t prim;           /* input triangle index, -1 = miss */
} bdpt_surface;           /* 96 bytes: six float4 */
#define BDPT_SHADE_NORMAL_MAP 1u
typedef struct bdpt_shade_desc {
  const bdpt_ray* rays;          /* device, 16-byte aligned, numHits records: only the origin is read */
  const bdpt_hit* hits;          /* device, 16-byte aligned, numHits records (e.g. bdpt_trace_rays' output) */
  uint32_t numHits;              /* hits to shade; the capacity when numHitsDevice is set */
  uint32_t flags;                /* BDPT_SHADE_* */
  const uint32_t* numHitsDevice; /* optional device word: shade min(*numHitsDevice, numHits) hits */
  bdpt_surface* surfaces;        /* device, 16-byte aligned, one per hit */
} bdpt_shade_desc;
int bdpt_shade_hits(bdpt_ctx* ctx, const bdpt_shade_desc* desc, void* stream);

/* bdpt_bsdf_query: the pass's BSDF at shaded records (read: N, V, diffuse, specular, linearRoughness, prim), the GGX model
 * (matIndex 0) or the Lambertian one (1), as bdpt_params::matIndex selects for the walk.
 *   BDPT_BSDF_SAMPLE  sampleBRDF(seeds[i], N, N, V, ...): the sampled direction, its pdf, the weight f * cos / pdf and
 *                     whether the lobe counts as specular (flags BDPT_PARAM_SPECULAR_FROM_LOBE as for the walk; without
 *                     it never).  The seed is read by value and not advanced.  pdf 0 with
 *                     a zero weight where the sample lies below the surface.
 *   BDPT_BSDF_EVAL    evalBRDF(V, L, N, N, ...) toward dirs[i] = (L.xyz, w): w != 0 evaluates the specular lobe (the
 *                     pass passes the flag its sample returned); values[i] = (f.xyz, 0).
 * A record with prim < 0 gives all-zero outputs.  With numDevice set, items at or beyond min(*numDevice, num) are neither
 * read nor written.
 * Record contract (tests/edge_records.py has the families, DESIGN.md "Surface queries" the measurements): every float
 * field may be degenerate or non-finite; none reaches an address, and the outputs are those of the fp32 arithmetic as
 * written, bit for bit the CPU oracle's.  N and V are used as given (a non-unit N scales the cosines).  Under GGX a V in
 * or below the tangent plane (saturate(N.V) = 0) makes the specular lobe's weight and f NaN (0 / 0) and leaves the diffuse
 * lobe alone; a linearRoughness whose fourth power underflows to 0 (below some 5e-12) gives the specular sample pdf 0 with
 * a NaN weight; dirs[i] == -V evaluates the specular lobe as NaN where N.L > 0 (the half vector is normalize(0)); N.L == 0
 * counts as below the surface (f = 0; a sample: pdf 0, weight 0).  A NaN or infinite colour channel stays in its channel
 * of f; in a sample it also reaches probDiffuse, and a NaN probDiffuse picks the specular lobe.  The caller's
 * clampVec(x, clampUpper) turns a NaN, a negative number and -inf into +0 and +inf into clampUpper, so such a weight
 * ends a path or saturates it; it cannot poison a sum. */
#define BDPT_BSDF_SAMPLE 0u
#define BDPT_BSDF_EVAL 1u
typedef struct bdpt_bsdf_sample {
  float dir[3];
  float pdf;
  float weight[3];
  uint32_t specular; /* 1: the sampled lobe counts as specular */
} bdpt_bsdf_sample;  /* 32 bytes */
typedef struct bdpt_bsdf_desc {
  const bdpt_surface* surfaces; /* device, 16-byte aligned, num records */
  uint32_t num;                 /* items; the capacity when numDevice is set */
  uint32_t mode;                /* BDPT_BSDF_* */
  const uint32_t* numDevice;    /* optional device word: min(*numDevice, num) items */
  uint32_t matIndex;            /* 0 GGX, 1 Lambertian */
  uint32_t flags;               /* BDPT_PARAM_SPECULAR_FROM_LOBE or 0 */
  const uint32_t* seeds;        /* SAMPLE: device, one RNG state per item */
  bdpt_bsdf_sample* samples;    /* SAMPLE: device, 16-byte aligned, one per item */
  const float* dirs;            /* EVAL: device, 16-byte aligned, four floats per item */
  float* values;                /* EVAL: device, 16-byte aligned, four floats per item */
} bdpt_bsdf_desc;
int bdpt_bsdf_query(bdpt_ctx* ctx, const bdpt_bsdf_desc* desc, void* stream);

/* ---- Motion: where a surface point was in the previous frame ----
 * bdpt_keep_pose                 gSkinnedPrevPositions of SkinningCache (ComputeSkinning.cs.slang): the pose before this
 *                                frame's updates, kept on the device — here for bdpt_update_geometry and
 *                                bdpt_update_skinned alike, per triangle corner.
 * bdpt_gbuffer_execute_motion    bdpt_gbuffer_execute plus one RGBA32F channel: the hit point's position in that pose.
 * bdpt_motion_query              the same for a caller's bdpt_hit records.
 * bdpt_bmfr_execute_motion       bdpt_bmfr_execute reprojecting through that channel ("BMFR denoiser" below).
 * The reference has no counterpart past the first: its BMFR reprojects the current position, so a moving surface
 * restarts at 1 spp every frame.  Every existing call keeps its bits; all of this is behind these entry points.
 *
 * bdpt_prepare(BDPT_PREPARE_MOTION) (needs a scene, not a size; allocates and synchronises, so not inside a stream capture:
 * BDPT_E_STATE) allocates the previous pose — three float4 per primitive, the corners p0, p1, p2 in primitive order, 48 B
 * per primitive — and fills it from the current shading records: previous == current.  bdpt_set_scene drops it.
 *
 * bdpt_keep_pose copies the current corner positions into the previous pose: one streaming kernel, enqueued on `stream`
 * behind the context's previous call (the event rule of bdpt_update_geometry); no allocation, no synchronise, one kernel
 * node in a captured graph; it always runs (a replayed graph replays it).  A caller calls it once per frame BEFORE that
 * frame's updates — also in a frame without an update: that is how an object that stops gets zero motion.  Updates
 * themselves do not touch the previous pose: two updates without a bdpt_keep_pose between them leave it alone.
 *
 * The previous position of a hit (prim, u, v) with the previous-pose corners p0, p1, p2, per component, fp32, no
 * contraction, exactly in this order (the arithmetic of the G-buffer's WorldPosition on the current corners, so an
 * unmoved scene gives WorldPosition's bits):
 *   b0 = 1 - u - v          prev = ((0 + p0*b0) + p1*u) + p2*v
 *
 * bdpt_gbuffer_execute_motion: bdpt_gbuffer_execute, and prevPosition (device, 16-byte aligned, width x height float4
 * texels in frame order) written for the context's tile pixels: (prev.xyz, 1) at a hit, (0, 0, 0, 0) at a miss, as
 * WorldPosition.  The six channels and the occluder hints get the bits bdpt_gbuffer_execute gives.
 *
 * bdpt_motion_query: prevPositions[i] = (prev.xyz, 1) for hits[i]; a prim < 0 or one that is not a triangle of the scene
 * writes zeros; with numDevice set, items at or beyond min(*numDevice, num) are neither read nor written.  Ordering,
 * capture and counters as the surface queries: stream-ordered behind the context's previous call, no allocation, no
 * synchronise, bdpt_get_counters and bdpt_get_stage_times left alone; num == 0 returns BDPT_OK and does nothing.
 *
 * Errors (nothing is enqueued): no scene, or no bdpt_prepare(BDPT_PREPARE_MOTION) since the last bdpt_set_scene,
 * BDPT_E_STATE (bdpt_gbuffer_execute_motion also without camera or size); a NULL context, params, channels or desc, a
 * missing or misaligned buffer, a non-zero reserved BDPT_E_INVALID. */
int bdpt_keep_pose(bdpt_ctx* ctx, void* stream);
typedef struct bdpt_motion_desc {
  const bdpt_hit* hits;      /* device, 16-byte aligned, num records (e.g. bdpt_trace_rays' output) */
  uint32_t num;              /* items; the capacity when numDevice is set */
  uint32_t reserved;         /* 0 */
  const uint32_t* numDevice; /* optional device word: min(*numDevice, num) items */
  float* prevPositions;      /* device, 16-byte aligned, one float4 per item */
} bdpt_motion_desc;
int bdpt_motion_query(bdpt_ctx* ctx, const bdpt_motion_desc* desc, void* stream);

/* ---- Light queries: the pass's light sampling, for a caller's own integrator ----
 * bdpt_light_query closes the forward half of the query family ("Connection queries" below has the two bidirectional
 * strategies): with it a forward path tracer with next-event estimation (NEE: sampling a
 * light directly from a surface point) is camera rays -> trace -> shade -> light query -> trace(any) -> sample -> trace ...
 * on one stream, capturable, with no read-back.  Both modes run the device functions the pass runs, bit for bit
 * (DESIGN.md "Light queries"): the composed calls reproduce bdpt_execute's NEE-only frame.
 *
 * Ordering, capture, counters, num == 0 and numDevice: as the surface queries.  The call allocates nothing, with one
 * exception: with BDPT_PARAM_AREA_LIGHTS in flags the emitter table ("Area lights" above) is made as bdpt_execute makes it,
 * by bdpt_prepare(BDPT_PREPARE_AREA_LIGHTS) or by the first call that needs it, which then must not be inside a stream
 * capture (BDPT_E_STATE).
 * lightsCount, the pass's rule: numLights, or numLights + 1 with BDPT_PARAM_AREA_LIGHTS while the table's W > 0 (light
 * numLights is then the table); with no emitter or W == 0 the flag changes nothing, bit for bit.  matIndex (0 GGX,
 * 1 Lambertian) and minT play the roles of bdpt_params::matIndex and minT.
 *
 * BDPT_LIGHT_NEE: one next-event sample per item, the light part of a NEE term of the pass.  Inputs: surfaces[i] (read:
 *   posW, N, V, diffuse, specular, linearRoughness, prim; the BSDF's roughness is linearRoughness^2) and the RNG state
 *   seeds[i].  Draws: r = nextRand(state) picks light min((int)(r * lightsCount), lightsCount - 1); when that is the
 *   table, a, u1, u2 come from initRand(<state after r>, 0x41524541u) ("Area lights", NEE term).  samples[i]:
 *     ray     org = posW, tmin = minT, dir = L, tmax = the distance to the light (the table: d (1 - 1e-4))
 *     value   ggxDirect / lambertianDirect of a VISIBLE light with shadowMult = lightsCount: unweighted and unclamped.
 *             Throughput, strategy weight and the clamp stay with the caller, in the pass's order:
 *             clampVec((prevColor * value) / k, clampUpper)
 *     light   the sampled light (numLights: the table)
 *     status  BDPT_LIGHT_STATUS_NONZERO: value has a component that is not +-0 (a ray is worth tracing);
 *             BDPT_LIGHT_STATUS_HINT_OCCLUDED: the occluder hint found the light occluded (no ray is needed)
 *   A record with prim < 0 gives an all-zero sample and still takes its one draw.  seedsOut[i] (optional; may be seeds) is
 *   the state after r: chaining it reproduces "term t uses the (t+1)-th draw after seedL".
 *   BDPT_LIGHT_USE_HINTS: for a point or spot light whose value has a positive component, the nearest triangle the light
 *   sees towards posW (the context's light cube maps) is tested first, exactly as the pass tests it; on success
 *   HINT_OCCLUDED is set.  A value that is not +-0 but has no positive component (NaN where dot(N, V) <= 0 under GGX, or a
 *   negative intensity) keeps NONZERO and is not tried: clampVec turns it into zero whatever the throughput and weight,
 *   so the pass, which tests its clamped term, never tries it either.
 *   Directional lights and the table never use hints.  A hint only ever saves a ray: visibility answers do not change.
 *   Compaction (compactRays, compactItems and compactCount, all or none): every item whose status is exactly NONZERO appends
 *   its ray to compactRays and its index to compactItems at a position taken from *compactCount (one atomic per wave of 64
 *   items).  The caller zeroes the word before the call and owns capacity num of both lists; the order inside the lists is
 *   unspecified.  compactRays / compactCount go straight to bdpt_trace_rays (BDPT_TRACE_ANY, numRaysDevice = compactCount).
 *   Without compaction the caller traces all num rays and masks by status.
 *
 * BDPT_LIGHT_EMIT: the start of a light subpath per item (sampleLight).  Input: seeds[i]; no surfaces.  Draws: the
 *   selection draw; then sampleUnitSphere (three draws per rejection round; not for directional lights, which start from
 *   dirW) and getCosHemisphereSample (two draws) around that direction; for the table a, u1, u2, the side and the cosine
 *   direction ("Area lights", light subpath start: six draws).  emits[i]:
 *     ray     org = lightPath[0].pos, tmin = minT, dir = the sampled direction, tmax = 1e38
 *     color   lightPath[0].color: the light's intensity, or Le * 2 pi / p_A for the table
 *     light   the sampled light
 *   lightPath[0].pdfForward is 1 / lightsCount and is not stored.  seedsOut[i] (optional) is the state after all draws: the
 *   pass's seedL.
 *
 * Record contract (tests/edge_records.py, DESIGN.md "Light queries"): the floats of a record and of a light may be
 * degenerate or non-finite; the scene has at least one light, and the light index, a draw in [0, 1) times lightsCount
 * clamped to lightsCount - 1, is in range whatever the record holds.  The outputs are the fp32 arithmetic's, bit for bit
 * the CPU oracle's:
 *   - a point within sqrt(1e-5) of a point or spot light (getLightData's switch), or so far that the squared distance
 *     overflows: dir is NaN and value is 0 (status 0), tmax the distance (0 at the light itself, inf beyond 1.8e19);
 *   - cosTheta == cosOpeningAngle is inside the cone; penumbraAngle > 0 scales by saturate((delta - p) / p), so a penumbra
 *     at or above openingAngle gives 0; acos is taken of cosTheta clamped to [-1, 1] (a build definition: HLSL leaves acos
 *     outside the interval to the driver), so a dirW longer than 1 widens the cone's bright core, never makes a NaN;
 *   - a zero dirW: a spot light sees cosTheta 0 everywhere; a directional light gives a NaN direction and value 0, and in
 *     EMIT a zero direction;
 *   - N.L <= 0, V below the surface or V == -L under GGX: value NaN (0 / 0) or 0; status NONZERO for the NaN, and no hint;
 *   - intensities pass through: negative ones give negative values, inf gives inf or NaN, none gets a hint unless some
 *     component is positive.
 *   A hint is looked up only for a value with a positive component, which implies a finite direction and distance: the
 *   cube map is indexed by a finite, non-zero posW - lightPos.  clampVec (see bdpt_bsdf_query) makes +0 of every NaN and
 *   negative value.
 *
 * Errors (nothing is enqueued): no scene BDPT_E_STATE; a NULL context or desc, an unknown mode or flag, matIndex > 1, a
 * missing or misaligned buffer (records 16 bytes, words 4), compaction buffers given in part, compaction or hints in EMIT
 * mode BDPT_E_INVALID. */
#define BDPT_LIGHT_NEE 0u
#define BDPT_LIGHT_EMIT 1u
#define BDPT_LIGHT_USE_HINTS 1u /* flags, beside BDPT_PARAM_AREA_LIGHTS */
#define BDPT_LIGHT_STATUS_NONZERO 1u
#define BDPT_LIGHT_STATUS_HINT_OCCLUDED 2u
typedef struct bdpt_light_sample {
  bdpt_ray ray;
  float value[3];
  uint16_t light;
  uint16_t status; /* BDPT_LIGHT_STATUS_* */
} bdpt_light_sample; /* 48 bytes: three float4 */
typedef struct bdpt_light_emit {
  bdpt_ray ray;
  float color[3];
  uint32_t light;
} bdpt_light_emit; /* 48 bytes: three float4 */
typedef struct bdpt_light_desc {
  uint32_t mode;                /* BDPT_LIGHT_* */
  uint32_t num;                 /* items; the capacity when numDevice is set */
  const uint32_t* numDevice;    /* optional device word: min(*numDevice, num) items */
  uint32_t matIndex;            /* NEE: 0 GGX, 1 Lambertian */
  uint32_t flags;               /* BDPT_PARAM_AREA_LIGHTS, BDPT_LIGHT_USE_HINTS (NEE) or 0 */
  float minT;                   /* tmin of the rays and of the hint test (bdpt_params::minT) */
  uint32_t reserved;
  const bdpt_surface* surfaces; /* NEE: device, 16-byte aligned, num records */
  const uint32_t* seeds;        /* device, one RNG state per item */
  uint32_t* seedsOut;           /* optional: device, one state per item */
  bdpt_light_sample* samples;   /* NEE: device, 16-byte aligned, one per item */
  bdpt_light_emit* emits;       /* EMIT: device, 16-byte aligned, one per item */
  bdpt_ray* compactRays;        /* NEE, optional: device, 16-byte aligned, capacity num */
  uint32_t* compactItems;       /* NEE, with compactRays: device, capacity num */
  uint32_t* compactCount;       /* NEE, with compactRays: device word, zeroed by the caller */
} bdpt_light_desc;
int bdpt_light_query(bdpt_ctx* ctx, const bdpt_light_desc* desc, void* stream);

/* ---- Connection queries: vertex pairs, camera splats and splat accumulation, for a caller's own integrator ----
 * The two strategies of the pass that join a light subpath to the eye side.  With the queries above every strategy is a
 * sequence of calls on one stream: the composed calls reproduce bdpt_execute's connection-only and splat-only frames bit for
 * bit (DESIGN.md "Connection queries").  Both calls run the device functions the pass runs (csrc/device_connect.hpp).
 *
 * Ordering, capture, counters, num == 0 and numDevice: as the surface queries — enqueued on `stream` behind the context's
 * previous call; no allocation and no synchronise (one kernel node in a captured graph); bdpt_get_counters and
 * bdpt_get_stage_times are left alone; items at or beyond min(*numDevice, num) are neither read nor written.
 * matIndex (0 GGX, 1 Lambertian) and minT play the roles of bdpt_params::matIndex and minT; the BSDF's roughness is
 * linearRoughness^2 as in bdpt_bsdf_query.  Vertices are bdpt_surface records (read: posW, N, diffuse, specular,
 * linearRoughness, prim, and V where stated; Lambertian reads neither V nor specular).
 *
 * BDPT_CONNECT_VERTICES: eye vertex eye[i] against light vertex light[i] (gen_connect's ev and le).
 *   eyePrev / lightPrev (optional, four floats per item, xyz used): the positions of the two predecessors; the outgoing
 *     directions are then normalize(prev - posW), as the pass forms woE and woL.  Without them the record's V is used: the
 *     same bits for a real vertex, not for the walk's ghost vertices (a copy of their predecessor).
 *   eyeSpecular / lightSpecular (optional bytes): bdpt_bsdf_sample::specular of the sample that left the vertex.  NULL
 *     means 0, which is what the pass uses without BDPT_PARAM_SPECULAR_FROM_LOBE.
 *   samples[i]:
 *     ray     org = eye.posW, tmin = minT, tmax = length(light.posW - eye.posW), dir = (light.posW - eye.posW) / tmax,
 *             written whatever prim says.  Coincident points give tmax 0 and a NaN direction: bdpt_trace_rays answers
 *             "miss", i.e. unoccluded for BDPT_TRACE_ANY, as the pass's lazy rounds rely on.
 *     value   (fsL * G) * fsE with fsL = evalBRDF(connectDir, woL, ...) at the light vertex, fsE = evalBRDF(-connectDir,
 *             woE, ...) at the eye vertex, connectDir = normalize(eye.posW - light.posW), G = evalGWithoutV.  The pass's
 *             short cuts are kept: fsL all zero gives fsL, then fsE all zero gives fsE.  All zero when either prim < 0.
 *             Unweighted and unclamped: the caller applies, in the pass's order,
 *             clampVec(w((aL * value) * aE), clampUpper), then NaN -> 0.  MIS prefix products are not provided.
 *     status  BDPT_CONNECT_STATUS_NONZERO: value has a component that is not +-0
 *
 * BDPT_CONNECT_CAMERA: light vertex light[i] against the context's camera (gen_splat without the path buffers), for a
 *   width x height frame with pixelJitter as in bdpt_params — always the whole frame, as bdpt_camera_rays.  Reads V (the
 *   walk's stored direction to the predecessor) and lightSpecular.  cameraSamples[i]:
 *     ray     org = posW, dir = normalize(camPos - posW), tmin = minT, tmax = length(camPos - posW)
 *     f       evalBRDF(V, dir, N, N, ...)
 *     G       saturate(|dot(dir, cameraN)|) * saturate(|dot(dir, N)|) / tmax^2.  f and G stay apart because the pass forms
 *             (prevColor * f) * G, which is not prevColor * (f * G) in fp32.
 *     pixel   x + y * width of the target (getLaunchIndexFromDirection with rintf(p * size - jitter))
 *     status  BDPT_CONNECT_STATUS_PIXEL: the vertex faces the camera (dot(cameraN, dir) < 0) and the target lies inside the
 *             frame; otherwise pixel = 0xffffffff and f = G = 0.  BDPT_CONNECT_STATUS_NONZERO (informational): f has a
 *             non-zero component and G != 0.
 *   prim < 0 gives an all-zero sample with pixel = 0xffffffff.  There are no occluder hints: those belong to the context's
 *   own G-buffer pass, and a hint only ever saves a ray.
 *
 * Compaction (compactRays, compactItems, compactCount: all or none) works as in bdpt_light_query: VERTICES appends the
 * items whose status has NONZERO, CAMERA those with PIXEL (the pass traces those whatever their value: a zero-valued splat
 * still saturates its pixel in the resolve).  One atomic per wave of 64 items; the caller zeroes the word and owns capacity
 * num of both lists; a position at or beyond num is not written; the order inside the lists is unspecified.
 *
 * Record contract (tests/edge_records.py, DESIGN.md "Connection queries"): every float of a record may be degenerate or
 * non-finite; the outputs are the fp32 arithmetic's, bit for bit the CPU oracle's.
 *   VERTICES: coincident points give tmax 0, a NaN direction and a NaN value (status NONZERO; the caller's clamp drops
 *   it) unless a cosine test made it 0 first; points closer than 1e-19 (invLengthAB^2 overflows) give inf or NaN, farther
 *   than 1.8e19 (length^2 overflows) tmax inf, a zero direction and 0 (Lambertian) or NaN (GGX, 0 / 0), as do two normals
 *   perpendicular to the connection; a predecessor equal to its vertex gives a NaN outgoing direction: NaN under GGX where
 *   that vertex's specular flag is set, else its diffuse lobe (a NaN passes the cosine test), as for Lambertian.
 *   CAMERA: the pixel is written only after 0 <= rintf(p * size - jitter) < size held for both coordinates, which fails
 *   for NaN and +-inf: pixel is below width * height or 0xffffffff, whatever the record holds.  rintf rounds a tie to the
 *   even pixel; -0.0 is pixel 0; a vertex in the camera plane or behind it (dot(cameraN, dir) >= 0), at the camera (a NaN
 *   direction) or beyond 1.8e19 (a zero direction) has no pixel.  f may be NaN with a pixel (GGX, V below the surface):
 *   the pass's NaN -> 0 and bdpt_splat_add's "c > 0" both drop it, and the splat still counts.
 *
 * Errors (nothing is enqueued): no scene, or CAMERA without a camera BDPT_E_STATE; a NULL context or desc, an unknown mode,
 * non-zero flags or reserved, matIndex > 1, a missing or misaligned buffer (records 16 bytes, words 4), compaction buffers
 * given in part, CAMERA with a width or height of 0 or width * height >= 2^32 BDPT_E_INVALID. */
#define BDPT_CONNECT_VERTICES 0u
#define BDPT_CONNECT_CAMERA 1u
#define BDPT_CONNECT_STATUS_NONZERO 1u
#define BDPT_CONNECT_STATUS_PIXEL 2u
typedef struct bdpt_connect_sample {
  bdpt_ray ray;
  float value[3];
  uint32_t status; /* BDPT_CONNECT_STATUS_NONZERO or 0 */
} bdpt_connect_sample; /* 48 bytes: three float4 */
typedef struct bdpt_camera_sample {
  bdpt_ray ray;
  float f[3];
  float G;
  uint32_t pixel;  /* x + y * width, 0xffffffff = none */
  uint32_t status; /* BDPT_CONNECT_STATUS_* */
  uint32_t reserved[2];
} bdpt_camera_sample; /* 64 bytes: four float4 */
typedef struct bdpt_connect_desc {
  uint32_t mode;                     /* BDPT_CONNECT_* */
  uint32_t num;                      /* items; the capacity when numDevice is set */
  const uint32_t* numDevice;         /* optional device word: min(*numDevice, num) items */
  uint32_t matIndex;                 /* 0 GGX, 1 Lambertian */
  uint32_t flags;                    /* 0 */
  float minT;                        /* tmin of the rays (bdpt_params::minT) */
  uint32_t reserved;                 /* 0 */
  const bdpt_surface* eye;           /* VERTICES: device, 16-byte aligned, num records */
  const bdpt_surface* light;         /* device, 16-byte aligned, num records */
  const float* eyePrev;              /* VERTICES, optional: device, 16-byte aligned, four floats per item */
  const float* lightPrev;            /* VERTICES, optional: device, 16-byte aligned, four floats per item */
  const uint8_t* eyeSpecular;        /* VERTICES, optional: device, one byte per item */
  const uint8_t* lightSpecular;      /* optional: device, one byte per item */
  bdpt_connect_sample* samples;      /* VERTICES: device, 16-byte aligned, one per item */
  bdpt_camera_sample* cameraSamples; /* CAMERA: device, 16-byte aligned, one per item */
  uint32_t width, height;            /* CAMERA: the frame */
  float pixelJitter[2];              /* CAMERA: bdpt_params::pixelJitter */
  bdpt_ray* compactRays;             /* optional: device, 16-byte aligned, capacity num */
  uint32_t* compactItems;            /* with compactRays: device, capacity num */
  uint32_t* compactCount;            /* with compactRays: device word, zeroed by the caller */
} bdpt_connect_desc;
int bdpt_connect_query(bdpt_ctx* ctx, const bdpt_connect_desc* desc, void* stream);

/* bdpt_splat_add: the splat half of the pass's gather for a caller's lists.  Entry j (of num, or of min(*numDevice, num))
 * uses item k = items ? items[j] : j: it reads pixels[k], values[k] (xyz: the clamped term) and visible[j], so CAMERA mode's
 * compact lists and bdpt_trace_rays' `visible` bytes go in as they are.  An entry lands when visible is NULL or
 * visible[j] != 0 and pixels[k] < numPixels.  A landed entry adds (uint64_t)(c * 2^32) to word 0 / 1 / 2 of
 * splat[pixels[k]] for each channel c > 0 (a NaN or non-positive channel adds nothing; a channel above
 * BDPT_MAX_CLAMP_UPPER_SPLAT is the caller's error: its conversion is undefined) and 1 to word 3, with 64-bit atomic
 * adds: integer sums, so the result is exact and does not depend on the order.  `splat` is a device buffer of uint64[4]
 * per pixel in frame order: the context's own (bdpt_splat_buffer of a whole-frame context) or the caller's, which
 * bdpt_resolve(ctx, splat, 0, out) folds in as it does the pass's.  Owner-major (stripes) layouts are not supported.
 * Ordering, capture, counters, num == 0: as above.  Needs no scene.  Errors (nothing is enqueued): a NULL context or desc, a
 * missing or misaligned buffer (splat and values 16 bytes, words 4) BDPT_E_INVALID. */
typedef struct bdpt_splat_desc {
  uint32_t num;              /* entries; the capacity when numDevice is set */
  uint32_t numPixels;        /* pixels of `splat` */
  const uint32_t* numDevice; /* optional device word: min(*numDevice, num) entries */
  const uint32_t* pixels;    /* device, one target per item (bdpt_camera_sample::pixel) */
  const float* values;       /* device, 16-byte aligned, four floats per item */
  const uint8_t* visible;    /* optional: device, one byte per entry */
  const uint32_t* items;     /* optional: device, one item index per entry */
  uint64_t* splat;           /* device, 16-byte aligned, uint64[4] per pixel */
} bdpt_splat_desc;
int bdpt_splat_add(bdpt_ctx* ctx, const bdpt_splat_desc* desc, void* stream);

/* ---- Walk queries: whole subpaths from one persistent kernel, for a caller's own integrator ----
 * bdpt_walk_query walks one subpath per item for up to `steps` bounces in one launch: shootRay and the closest-hit
 * shader of the reference's two walks (BDPT/BDPTMain.rt.hlsl:106-145, BDPT/globalIlluminationRay.hlsli:1-45).  It is the
 * loop bdpt_trace_rays(BDPT_TRACE_CLOSEST) -> bdpt_shade_hits (without BDPT_SHADE_NORMAL_MAP) -> bdpt_bsdf_query(SAMPLE)
 * -> select the hits, multiply the colours, build the next rays, bit for bit, run with the device functions those calls
 * and the pass run, without a launch and a trip through memory per stage and bounce (DESIGN.md "Walk queries").
 *
 * State of item i: `payload`, a bdpt_surface, starting as first[i], or without `first` as posW = starts[i].ray.org with
 * every other word 0; `pspec`, starting as firstSpecular[i] != 0 (NULL: 0); `pcolor`, starting as starts[i].color; the
 * direction L, starting as starts[i].ray.dir; `live`, starting as alive ? alive[i] != 0 : true.
 * Step s = 0 .. steps-1 runs while `live` holds:
 *   - the ray is (payload.posW, L), traced as BDPT_TRACE_CLOSEST traces it; step 0 takes tmin and tmax from starts[i].ray,
 *     later steps minT and 1e38;
 *   - a hit is shaded as bdpt_shade_hits shades it without the normal map, seen from the ray's origin, and the record is
 *     sampled as bdpt_bsdf_query(SAMPLE) samples it with matIndex and the BDPT_PARAM_SPECULAR_FROM_LOBE bit of `flags`.
 *     The seed is read by value and never advanced: every step uses seeds[i] (the reference's quirk, which the pass
 *     keeps); with BDPT_WALK_SEED_PER_STEP step s uses seeds[s * num + i], so a caller can decorrelate the bounces.  Then
 *     payload = the record, pspec = the sample's specular word, pcolor = pcolor * weight, L = the sampled direction, and
 *     the vertex is REAL;
 *   - a miss — everything bdpt_trace_rays calls a miss: a NaN or zero direction, a NaN origin, tmax <= tmin — sets
 *     pcolor = +0 and makes the vertex a ghost: payload and pspec stay as they were, and the walk ends after this step
 *     (RayMiss: the ghost and the last direction are what a caller needs for an environment term);
 *   - vertex s is written: vertices[s * num + i] = payload with prim = max(prim, 0), info.color = pcolor, info.status =
 *     STORED, plus REAL for a real vertex, plus SPECULAR where pspec is set.  A real vertex writes the sample drawn at it
 *     to `samples` and (t, u, v, prim) to `hits`; a ghost writes zeros to both, with hits.prim = -1.
 * Steps after the walk has ended, and every step of an item that is not alive, write an all-zero record with prim = -1,
 * colour +0 and status 0, and fill a given `samples` and `hits` as for a ghost.
 *
 * bdpt_light_query(BDPT_LIGHT_EMIT)'s output goes in as `starts` unchanged for a light walk (the last word is not read).
 * An eye walk starts from the G-buffer vertex as `first`, with its first sample's direction and weight in `starts`; or
 * straight from bdpt_camera_rays with a colour of 1 (step 0 then takes the camera ray's tmin and tmax), in which case the
 * primary hit is shaded without the normal map, unlike the G-buffer pass's.
 *
 * Ordering, capture, counters and numDevice: as the surface queries — enqueued on `stream` behind the context's previous
 * call, which also keeps bdpt_trace_rays' INVARIANT (no two persistent traversal kernels of one context resident at
 * once); no allocation and no synchronise (one kernel node in a captured graph); bdpt_get_counters and
 * bdpt_get_stage_times are left alone; items at or beyond min(*numDevice, num) are neither read nor written, and the plane
 * stride stays num.  Nothing a caller supplies reaches an address: prim comes from the traversal only, `first` is copied.
 * The ray and record contracts of bdpt_trace_rays and bdpt_bsdf_query hold for every step.
 * Errors (nothing is enqueued): no scene BDPT_E_STATE; a NULL context or desc, steps of 0 or above BDPT_MAX_DEPTH,
 * matIndex > 1, unknown flags, a non-zero reserved, steps * num >= 2^32 BDPT_E_INVALID; then num == 0 returns BDPT_OK
 * and does nothing; then a missing or misaligned buffer (records 16 bytes, words 4) BDPT_E_INVALID. */
#define BDPT_WALK_SEED_PER_STEP 1u   /* flags, beside BDPT_PARAM_SPECULAR_FROM_LOBE */
#define BDPT_WALK_STATUS_STORED 1u   /* the vertex exists: a real vertex or a ghost */
#define BDPT_WALK_STATUS_REAL 2u     /* made by a hit */
#define BDPT_WALK_STATUS_SPECULAR 4u /* the specular byte the pass keeps for this vertex */
typedef struct bdpt_walk_start {
  bdpt_ray ray;
  float color[3];
  uint32_t unused; /* not read (bdpt_light_emit::light) */
} bdpt_walk_start; /* 48 bytes: bdpt_light_emit's layout */
typedef struct bdpt_walk_info {
  float color[3];
  uint32_t status; /* BDPT_WALK_STATUS_* */
} bdpt_walk_info;  /* 16 bytes */
typedef struct bdpt_walk_desc {
  uint32_t num;                  /* items; the capacity when numDevice is set */
  uint32_t steps;                /* 1 .. BDPT_MAX_DEPTH */
  const uint32_t* numDevice;     /* optional device word: min(*numDevice, num) items */
  uint32_t matIndex;             /* 0 GGX, 1 Lambertian */
  uint32_t flags;                /* BDPT_PARAM_SPECULAR_FROM_LOBE, BDPT_WALK_SEED_PER_STEP or 0 */
  float minT;                    /* tmin of the rays after step 0 (bdpt_params::minT) */
  uint32_t reserved;             /* 0 */
  const bdpt_walk_start* starts; /* device, 16-byte aligned, num records */
  const uint32_t* seeds;         /* device, num RNG states, or steps x num with BDPT_WALK_SEED_PER_STEP */
  const bdpt_surface* first;     /* optional: device, 16-byte aligned, num records: the predecessor a step-0 ghost copies */
  const uint8_t* firstSpecular;  /* optional: device, one byte per item (NULL = 0) */
  const uint8_t* alive;          /* optional: device, one byte per item, 0 = the item has no path */
  bdpt_surface* vertices;        /* device, 16-byte aligned, steps x num records, [s * num + i] */
  bdpt_walk_info* info;          /* device, 16-byte aligned, steps x num records */
  bdpt_bsdf_sample* samples;     /* optional: device, 16-byte aligned, steps x num records */
  bdpt_hit* hits;                /* optional: device, 16-byte aligned, steps x num records */
} bdpt_walk_desc;
int bdpt_walk_query(bdpt_ctx* ctx, const bdpt_walk_desc* desc, void* stream);

/* ---- Ambient occlusion: S cosine-weighted any-hit rays per item inside a radius, from one persistent kernel ----
 * bdpt_ao_query is the reference's AO ray generation shader on a caller's items
 * (CommonPasses/Data/CommonPasses/aoTracing.rt.hlsl:74-122); bdpt_ao_execute is its pass on the G-buffer
 * (CommonPasses/AmbientOcclusionPass.cpp:76-96).  It is the loop, per sample, bdpt_bsdf_query(SAMPLE, matIndex 1) -> build
 * the rays -> bdpt_trace_rays(BDPT_TRACE_ANY) -> add the visibility bytes, bit for bit, run with the device functions
 * those calls run, without two launches and a trip through memory per sample (DESIGN.md "Ambient occlusion").
 *
 * Item i is alive iff surfaces[i].prim >= 0 and (alive == NULL or alive[i] != 0).  For an alive item:
 *   s = seeds[i]; count = 0;
 *   for k = 0 .. samples-1: dir = getCosHemisphereSample(s, N) — two draws, s advances (the Lambertian sampleBRDF's
 *     direction: BDPT/MaterialUtils.hlsli:41-54); the ray is org = posW, tmin = minT, dir, tmax = radius, traced as
 *     BDPT_TRACE_ANY traces it (the alpha test included, a hit needs tmin < t < tmax); count += 1 when it is unoccluded;
 *   ao[i] = (float)count / (float)samples, a correctly rounded fp32 division (aoTracing.rt.hlsl:121); counts[i] = count;
 *   seedsOut[i] = s, the state after exactly 2 * samples draws.
 * A dead item gives ao = 1, counts = samples and seedsOut = seeds[i] with no draw (the shader's background branch,
 * aoTracing.rt.hlsl:88-91).  seedsOut may be `seeds`.  `counts` lets a caller accumulate over frames exactly.
 * radius and minT are not validated; they follow the ray contract of bdpt_trace_rays: radius <= minT, or a NaN in
 * either, makes every ray a miss, so ao = 1.
 * Record contract: only posW, N and prim are read, and prim only for its sign: it reaches no address.  N need not be
 * unit, finite or non-zero, posW need not be finite: the direction is that of the fp32 arithmetic as written
 * (bdpt_bsdf_query's record contract), and a zero or NaN direction or a NaN origin is a miss under the ray contract, so a
 * record with N = 0, a NaN in N or a NaN in posW gives ao = 1 after its 2 * samples draws.  A normal so short that a
 * component of the direction falls below 1e-30 comes under that rule of the ray contract.  ao is always in [0, 1].
 *
 * bdpt_ao_execute runs the same for the context's tile pixels (rows or stripes), reading the FULL-FRAME G-buffer
 * channels worldPosition and worldNormal and writing `out` (full-frame RGBA32F, addressed as bdpt_execute addresses it)
 * at the tile's pixels only: pixel (x, y) has seed initRand(x + y * width, frameCount, 16) with the full frame's width
 * and the absolute y (aoTracing.rt.hlsl:82), so tiles reproduce the whole frame; it is alive iff worldPosition.w != 0;
 * N is the half-decoded xyz of worldNormal; out = (ao, ao, ao, 1).  It needs a scene and a size, not a camera.
 *
 * Ordering, capture, counters and numDevice: as the surface queries — enqueued on `stream` behind the context's previous
 * call, which also keeps bdpt_trace_rays' INVARIANT (no two persistent traversal kernels of one context resident at
 * once); no allocation and no synchronise (exactly one kernel node in a captured graph); bdpt_get_counters and
 * bdpt_get_stage_times are left alone; items at or beyond min(*numDevice, num) are neither read nor written.  Nothing a
 * caller supplies reaches an address.
 * Errors (nothing is enqueued), in this order: a NULL context, desc / params or gbuffer BDPT_E_INVALID; no scene
 * (bdpt_ao_execute: or no size) BDPT_E_STATE; samples outside 1 .. BDPT_AO_MAX_SAMPLES (the reference's GUI range,
 * AmbientOcclusionPass.cpp:69; 0 would be 0 / 0), non-zero flags or reserved BDPT_E_INVALID; then num == 0 returns BDPT_OK
 * and does nothing; then a missing or misaligned buffer BDPT_E_INVALID: records and `out` 16 bytes, worldNormal 8, words
 * (seeds, ao, counts, seedsOut, numDevice) 4; a NULL `out` is found here. */
#define BDPT_AO_MAX_SAMPLES 64u
typedef struct bdpt_ao_desc {
  uint32_t num;                 /* items; the capacity when numDevice is set */
  uint32_t samples;             /* 1 .. BDPT_AO_MAX_SAMPLES rays per item */
  const uint32_t* numDevice;    /* optional device word: min(*numDevice, num) items */
  float radius;                 /* tmax of the rays */
  float minT;                   /* tmin of the rays (bdpt_params::minT) */
  uint32_t flags;               /* 0 */
  uint32_t reserved;            /* 0 */
  const bdpt_surface* surfaces; /* device, 16-byte aligned, num records: posW, N and prim are read */
  const uint32_t* seeds;        /* device, num RNG states */
  const uint8_t* alive;         /* optional: device, one byte per item, 0 = the item is dead */
  float* ao;                    /* device, num floats */
  uint32_t* counts;             /* optional: device, num words: the unoccluded samples */
  uint32_t* seedsOut;           /* optional: device, num RNG states (may be `seeds`) */
} bdpt_ao_desc;
int bdpt_ao_query(bdpt_ctx* ctx, const bdpt_ao_desc* desc, void* stream);
typedef struct bdpt_ao_params {
  uint32_t frameCount; /* starts at 0 and grows by one per frame (AmbientOcclusionPass.h:54, .cpp:86) */
  float radius;        /* the pass's default: max(0.1, scene radius * 0.05) (AmbientOcclusionPass.cpp:62) */
  float minT;
  uint32_t samples;    /* 1 .. BDPT_AO_MAX_SAMPLES; the pass's default is 1 (AmbientOcclusionPass.h:55) */
  uint32_t reserved;   /* 0 */
} bdpt_ao_params;
int bdpt_ao_execute(bdpt_ctx* ctx, const bdpt_ao_params* p, const bdpt_gbuffer* gbuffer, float* out, void* stream);

/* ---- Diffuse GI: direct light plus one diffuse bounce per item, up to three rays, from one persistent kernel ----
 * bdpt_gi_query is the reference's one-bounce path tracer on a caller's items, the ray generation shader
 * SimpleDiffuseGIRayGen with its IndirectMiss / IndirectClosestHit pair
 * (CommonPasses/Data/CommonPasses/simpleDiffuseGI.rt.hlsl:61-108, 133-198); bdpt_gi_execute is its pass on the G-buffer
 * (CommonPasses/SimpleDiffuseGIPass.cpp:89-117).  It is the loop bdpt_light_query(NEE) -> bdpt_trace_rays(ANY) ->
 * bdpt_bsdf_query(SAMPLE) -> bdpt_trace_rays(CLOSEST) -> bdpt_shade_hits -> bdpt_light_query(NEE) -> bdpt_trace_rays(ANY)
 * and the arithmetic between them, bit for bit, run with the device functions those calls run, in one launch
 * (DESIGN.md "Diffuse GI").  kPi below is fp32 M_PI.
 *
 * Item i is alive iff surfaces[i].prim >= 0 and (alive == NULL or alive[i] != 0).  With s = seeds[i]:
 *   dead:  color = (diffuse.rgb, 1) (the shader's background branch, .hlsl:146-152), no draw, seedsOut = s, status = 0,
 *          hit = (0, 0, 0, -1).
 *   alive: (ray1, value1) = NEE(record, s): one draw, s advances: exactly bdpt_light_query(BDPT_LIGHT_NEE, matIndex 1,
 *            flags 0) on (record, s): the light choice, getLightData, value = (((lightsCount * LdotN) * I) * diffuse) / kPi
 *            with lightsCount = numLights (.hlsl:155-170)
 *          direct = term(value1, ray1); color = direct
 *          with BDPT_GI_INDIRECT:
 *            dir   = BDPT_GI_UNIFORM ? getUniformHemisphereSample(s, N) : getCosHemisphereSample(s, N), two draws
 *                    (.hlsl:176-180, simpleDiffuseGIUtils.hlsli:114-143)
 *            NdotL = saturate(dot(N, dir))
 *            hit   = the closest hit of (posW, minT, dir, 1e38) as BDPT_TRACE_CLOSEST answers it (alpha test included)
 *            miss: bounce = the context's environment toward dir (bdpt_set_environment: the map's lat-long texel, else the
 *                  constant colour; none = black) (IndirectMiss, .hlsl:61-73)
 *            hit:  rec = the hit shaded as bdpt_shade_hits shades it with `shadeFlags`, seen from `viewPos` with
 *                  BDPT_GI_SHADE_FROM_VIEW, else from the item's posW;
 *                  t = s, a copy (the payload's seed: the item's own state does not advance);
 *                  (ray2, value2) = NEE(rec, t); bounce = term(value2, ray2) (IndirectClosestHit, .hlsl:85-108)
 *            prob  = BDPT_GI_UNIFORM ? 1.0f / (2.0f * kPi) : NdotL / kPi
 *            color = direct + (((NdotL * bounce) * diffuse) / kPi) / prob, as written, nothing cancelled (.hlsl:189-192):
 *                    with cosine sampling NdotL = 0 gives 0 / 0 = NaN, as the shader does
 *          seedsOut = s (one draw without BDPT_GI_INDIRECT, three with); out = (color, 1)
 *   term(value, ray) = value when every component of value is +-0 (no ray is traced), else +0 when the ray is occluded as
 *                      BDPT_TRACE_ANY answers it, else value.
 * Build definitions: an occluded light contributes exactly +0 (directIfVisible's rule; the shader's 0 * inf would be NaN).
 * prob for uniform sampling is the fp32 expression above.  Falcor's prepareShadingData in getHitShadingData shades from
 * gCamera.posW, not from the ray origin, which decides the flip of double-sided normals: BDPT_GI_SHADE_FROM_VIEW is the
 * reference's behaviour, and bdpt_gi_execute always uses it with the context's camera position and shadeFlags =
 * BDPT_SHADE_NORMAL_MAP (full prepareShadingData applies the normal map).  mDoDirectShadows writes gDirectShadow, which
 * the shader never declares (SimpleDiffuseGIPass.cpp:103): it has no effect, and none here.  The emitter table and
 * occluder hints are not part of this call.
 * status bits: BDPT_GI_STATUS_DIRECT_OCCLUDED ray1 was traced and occluded; BDPT_GI_STATUS_BOUNCE_HIT the bounce ray hit;
 * BDPT_GI_STATUS_BOUNCE_OCCLUDED ray2 was traced and occluded.  hits[i] is the bdpt_hit of the bounce ray, (0, 0, 0, -1)
 * when there is none or it missed.
 * Record contract: posW, N, diffuse and prim are read, prim for its sign only: nothing a caller supplies reaches an
 * address.  The floats may be degenerate or non-finite; the results are those of the fp32 arithmetic as written, and a
 * zero or NaN direction or a NaN origin is a miss under the ray contract of bdpt_trace_rays, so such a bounce sees the
 * environment.
 *
 * bdpt_gi_execute runs the same for the context's tile pixels (rows or stripes), reading the FULL-FRAME G-buffer
 * channels worldPosition, worldNormal and materialDiffuse (halves decoded to fp32) and writing `out` (full-frame
 * RGBA32F) at the tile's pixels only: pixel (x, y) has seed initRand(x + y * width, frameCount, 16) with the full
 * frame's width and the absolute y (.hlsl:149); it is alive iff worldPosition.w != 0.  It needs a scene, a size and a
 * camera.
 *
 * Ordering, capture, counters and numDevice: as bdpt_ao_query — enqueued on `stream` behind the context's previous call,
 * which also keeps bdpt_trace_rays' INVARIANT; no allocation and no synchronise (exactly one kernel node in a captured
 * graph); bdpt_get_counters and bdpt_get_stage_times are left alone; items at or beyond min(*numDevice, num) are neither
 * read nor written.
 * Errors (nothing is enqueued), in this order: a NULL context, desc / params or gbuffer BDPT_E_INVALID; no scene
 * (bdpt_gi_execute: or no size, or no camera) BDPT_E_STATE; unknown flags (bdpt_gi_params: anything but INDIRECT |
 * UNIFORM), unknown shadeFlags or non-zero reserved BDPT_E_INVALID; then num == 0 returns BDPT_OK and does nothing; then
 * a missing or misaligned buffer BDPT_E_INVALID: records, color, hits and `out` 16 bytes, worldNormal and materialDiffuse
 * 8, words (seeds, status, seedsOut, numDevice) 4. */
#define BDPT_GI_INDIRECT 1u        /* gDoIndirectGI */
#define BDPT_GI_UNIFORM 2u         /* !gCosSampling */
#define BDPT_GI_SHADE_FROM_VIEW 4u /* bdpt_gi_query: shade the bounce hit as seen from viewPos */
#define BDPT_GI_STATUS_DIRECT_OCCLUDED 1u
#define BDPT_GI_STATUS_BOUNCE_HIT 2u
#define BDPT_GI_STATUS_BOUNCE_OCCLUDED 4u
typedef struct bdpt_gi_desc {
  uint32_t num;                 /* items; the capacity when numDevice is set */
  uint32_t flags;               /* BDPT_GI_* */
  const uint32_t* numDevice;    /* optional device word: min(*numDevice, num) items */
  uint32_t shadeFlags;          /* BDPT_SHADE_* for the bounce hit */
  float minT;                   /* tmin of every ray (bdpt_params::minT) */
  float viewPos[3];             /* read with BDPT_GI_SHADE_FROM_VIEW */
  uint32_t reserved;            /* 0 */
  const bdpt_surface* surfaces; /* device, 16-byte aligned, num records: posW, N, diffuse and prim are read */
  const uint32_t* seeds;        /* device, num RNG states */
  const uint8_t* alive;         /* optional: device, one byte per item, 0 = the item is dead */
  float* color;                 /* device, 16-byte aligned, num float4 */
  bdpt_hit* hits;               /* optional: device, 16-byte aligned, num records: the bounce ray's hit */
  uint32_t* status;             /* optional: device, num words of BDPT_GI_STATUS_* */
  uint32_t* seedsOut;           /* optional: device, num RNG states (may be `seeds`) */
} bdpt_gi_desc;
int bdpt_gi_query(bdpt_ctx* ctx, const bdpt_gi_desc* desc, void* stream);
typedef struct bdpt_gi_params {
  uint32_t frameCount; /* starts at 0x1337 and grows by one per frame (SimpleDiffuseGIPass.h:62, .cpp:100) */
  float minT;
  uint32_t flags;      /* BDPT_GI_INDIRECT | BDPT_GI_UNIFORM; the pass's defaults: INDIRECT, cosine (SimpleDiffuseGIPass.h:57-59) */
  uint32_t reserved;   /* 0 */
} bdpt_gi_params;
int bdpt_gi_execute(bdpt_ctx* ctx, const bdpt_gi_params* p, const bdpt_gbuffer* gbuffer, float* out, void* stream);

/* ---- Direct lighting: every light of the scene at every item, at most one any-hit ray each, from one persistent kernel ----
 * bdpt_direct_query is the reference's Lambertian-plus-shadows ray generation shader on a caller's items
 * (CommonPasses/Data/CommonPasses/lambertianPlusShadows.rt.hlsl:51-149); bdpt_direct_execute is its pass on the G-buffer
 * (CommonPasses/LambertianPlusShadowPass.cpp:64-83).  It is the only pass with no random draw: every light is evaluated
 * at every item, so one call is converged direct lighting, and there are no seeds in or out.  It replaces the loop, per
 * light, bdpt_set_lights(a one-light table) -> bdpt_light_query(NEE, matIndex 1) -> bdpt_trace_rays(BDPT_TRACE_ANY) -> an
 * accumulate, run with the device functions those calls run, in one launch (DESIGN.md "Direct lighting").
 *
 * Item i is alive iff surfaces[i].prim >= 0 and (alive == NULL or alive[i] != 0).
 *   dif   = diffuse;  if (dot(dif, dif) < 0.00001f) dif = specular                       (.hlsl:109-114)
 *   dead:   color = (dif, 1) (after the fallback), visible = 0, traced = 0               (.hlsl:117, 120)
 *   alive:  sum = (0, 0, 0)
 *           for k = 0 .. numLights-1, in this order:
 *             (L, I, dist) = getLightData(light k, posW)       Falcor ShadingUtils/Lights.slang:54-102, as every pass here
 *             LdotN = saturate(dot(N, L))                      NaN saturates to 0
 *             s_k   = 1.0f if the ray org = posW, tmin = minT, dir = L, tmax = dist is unoccluded as BDPT_TRACE_ANY
 *                     answers it (the alpha test included, a hit needs tmin < t < tmax), else 0.0f
 *             sum  += (s_k * LdotN) * I                                                   (.hlsl:140)
 *           color = (sum * (dif / 3.141592f), 1)    the shader's literal, not fp32 M_PI   (.hlsl:144)
 * A ray is not traced when it cannot change a bit of the result: when LdotN == 0 (which covers a NaN direction and a
 * point sitting at the light), or when every component of I is +-0 (as outside a spot light's cone).  In both cases
 * (0 * LdotN) * I and (1 * LdotN) * I are the same bits; the term is added as written with s_k = 1, so a non-finite
 * intensity gives the shader's NaN or inf.  bdpt_gi_query's rule "an occluded light contributes exactly +0" deliberately
 * does NOT apply here: this shader multiplies by its shadow factor, and so does the query: an occluded light of infinite
 * intensity gives 0 * inf = NaN.
 * Build definition: the shader's payload is an `int hitDist` initialised to maxT + 1.0f (.hlsl:60-75), which read as
 * written answers "visible iff no accepted hit" for 0 <= dist < 2^24 and otherwise leaves the answer to a float-to-int
 * conversion.  The build defines visibility as "no accepted hit in (minT, dist)" for every dist.
 *
 * Outputs: color (num float4) is required.  visible[i] (optional): bit k is set iff light k's term was added with
 * s_k = 1 — the ray was traced and unoccluded, or no ray was needed — so color can be recomputed under changed
 * intensities without tracing again.  traced[i] (optional): bit k is set iff a ray or a hint test was spent on light k.
 * BDPT_DIRECT_USE_HINTS: for a point or spot light whose term LdotN * I has a positive component, the nearest triangle
 * the light sees toward the item (the context's light cube map, as BDPT_LIGHT_USE_HINTS of bdpt_light_query) is tested
 * first; when it occludes the segment the term is settled with s_k = 0 and no traversal.  A hint only ever saves a
 * traversal: color, visible and traced are bit-identical with and without the flag.
 * The emitter table (BDPT_PARAM_AREA_LIGHTS) is not part of this call: the reference's pass has none, and sampling it
 * needs a draw; the flag is BDPT_E_INVALID.  Lights are those of the scene as bdpt_set_lights last left them.
 * Record contract: posW, N, diffuse, specular and prim are read, prim for its sign only: nothing a caller supplies
 * reaches an address.  The floats may be degenerate or non-finite; the results are those of the fp32 arithmetic as written,
 * and a zero or NaN direction or a NaN origin is a miss (s_k = 1) under the ray contract of bdpt_trace_rays.
 *
 * bdpt_direct_execute runs the same for the context's tile pixels (rows or stripes), reading the FULL-FRAME G-buffer
 * channels worldPosition, worldNormal, materialDiffuse and materialSpecRough (halves decoded to fp32) and writing `out`
 * (full-frame RGBA32F) at the tile's pixels only; a pixel is alive iff worldPosition.w != 0.  It needs a scene and a
 * size, not a camera.
 *
 * Ordering, capture, counters and numDevice: as bdpt_gi_query — enqueued on `stream` behind the context's previous call,
 * which also keeps bdpt_trace_rays' INVARIANT; no allocation and no synchronise (exactly one kernel node in a captured
 * graph); bdpt_get_counters and bdpt_get_stage_times are left alone; items at or beyond min(*numDevice, num) are neither
 * read nor written.
 * Errors (nothing is enqueued), in this order: a NULL context, desc / params or gbuffer BDPT_E_INVALID; no scene
 * (bdpt_direct_execute: or no size) BDPT_E_STATE; flags other than BDPT_DIRECT_USE_HINTS (BDPT_PARAM_AREA_LIGHTS among
 * them) or non-zero reserved BDPT_E_INVALID; then num == 0 returns BDPT_OK and does nothing; then a missing or misaligned
 * buffer BDPT_E_INVALID: records, color and `out` 16 bytes, the half channels 8, words (visible, traced, numDevice) 4. */
#define BDPT_DIRECT_USE_HINTS 1u
typedef struct bdpt_direct_desc {
  uint32_t num;                 /* items; the capacity when numDevice is set */
  uint32_t flags;               /* BDPT_DIRECT_USE_HINTS or 0 */
  const uint32_t* numDevice;    /* optional device word: min(*numDevice, num) items */
  float minT;                   /* tmin of every ray (bdpt_params::minT) */
  uint32_t reserved;            /* 0 */
  const bdpt_surface* surfaces; /* device, 16-byte aligned, num records: posW, N, diffuse, specular and prim are read */
  const uint8_t* alive;         /* optional: device, one byte per item, 0 = the item is dead */
  float* color;                 /* device, 16-byte aligned, num float4 */
  uint32_t* visible;            /* optional: device, num words, bit k: light k was added with s_k = 1 */
  uint32_t* traced;             /* optional: device, num words, bit k: a ray or a hint test was spent on light k */
} bdpt_direct_desc;
int bdpt_direct_query(bdpt_ctx* ctx, const bdpt_direct_desc* desc, void* stream);
typedef struct bdpt_direct_params {
  float minT;
  uint32_t flags;       /* BDPT_DIRECT_USE_HINTS or 0 */
  uint32_t reserved[2]; /* 0 */
} bdpt_direct_params;
int bdpt_direct_execute(bdpt_ctx* ctx, const bdpt_direct_params* p, const bdpt_gbuffer* gbuffer, float* out, void* stream);

/* ---- Environment lighting: a sampling table over the bound map, a sample / eval query, and a fused sky pass ----
 * The map of bdpt_set_environment is otherwise seen only by rays that happen to leave the scene (the G-buffer's miss
 * shader, BDPT_PARAM_ENV_ON_MISS, the diffuse GI kernel's IndirectMiss).  bdpt_env_prepare builds a discrete distribution
 * over its texels, bdpt_env_query samples it (next-event estimation) and evaluates directions against it (MIS for a
 * caller's BSDF-sampled miss), bdpt_sky_query / bdpt_sky_execute are the fused loop sample -> any-hit ray -> ordered add.
 * bdpt_execute does not change: environment NEE inside the BDPT frame is not part of this.  All arithmetic below is
 * csrc/env_light.h, one text compiled for the host (bdpt_host_env_*) and for the device, fp32 / fp64 as written, without
 * contraction; the table is exact in integers, so nothing depends on summation order.
 *
 * Table, for the W x H RGBA32F map, 1 <= W, H <= BDPT_ENV_MAX_DIM (beyond: BDPT_E_LIMIT):
 *   clean(c)  = c > 0 ? min(c, FLT_MAX) : 0                       NaN and negative channels count as 0
 *   lum(x, y) = (clean(r) * 0.2126f + clean(g) * 0.7152f) + clean(b) * 0.0722f (`luminance`); when a channel is positive
 *               and the sum rounds to 0 (subnormal channels), lum is the smallest subnormal: any positive channel gives lum > 0
 *   sinRow(y) = the sine of det_sincos2pi(((y + 0.5f) / H) * 0.5f), positive for every row
 *   f(x, y)   = min(lum * sinRow, FLT_MAX), and the smallest subnormal when lum > 0 and the product rounds to 0
 *   m         = max f over the map (order-free; on the device an unsigned atomicMax on the float's bits)
 *   q(x, y)   = f > 0 ? 1 + (uint32_t)(((double)f / (double)m) * 65535.0) : 0, in [0, 65536]: no lit texel is unreachable
 *   cdf[y][x] = inclusive prefix sum of q along row y (uint32; a row total is at most 2^30)
 *   rowCdf[y] = inclusive prefix sum of the row totals (uint64); total = rowCdf[H - 1] <= 2^44
 * Sample, envSample(state): exactly four draws r1 .. r4 of nextRand, in that order, whatever happens.
 *   total == 0: every output is zero.  Otherwise
 *   t  = min((uint64_t)((double)r1 * (double)total), total - 1);        y = the first row with rowCdf[y] > t
 *   t2 = min((uint32_t)((double)r2 * (double)rowTotal), rowTotal - 1);  x = the first column with cdf[y][x] > t2
 *   u = ((float)x + r3) / W, v = ((float)y + r4) / H; (s, c) = det_sincos2pi(u), (st, ct) = det_sincos2pi(v * 0.5f)
 *   dir = (-st * s, ct, st * c) — the inverse of envLookup's u = (1 + atan2_WAR(x, -z) / pi) / 2, v = acos(y) / pi
 *   radiance = the texel's rgb as stored; texel = y * W + x
 *   pdf = the solid-angle density (q / total) * (W * H) / (2 pi^2 st), evaluated as
 *         p = (float)((double)q / (double)total); pdf = ((p * (float)W) * (float)H) / ((2.0f * (kPi * kPi)) * st),
 *         and 0 when st <= 0.  Accuracy: within 1e-4 relative of the float64 reading of the formula wherever sin(pi v) is above
 *         2^-8; nearer a pole fp32 cannot hold it: v, a number up to 1 with two roundings behind it, is off by up to 1.2e-7,
 *         its sine by pi times that, which is more than 1e-4 of a sine below 3.7e-3.  The sin-weighted table puts under 1 %
 *         of any map's samples there (tests/test_env_cpu.py asserts the share).
 *   Build definition: a draw has 24 bits, so it picks among at most 2^24 targets: a row or a texel whose probability is
 *   below 2^-24 may never be drawn, although its pdf is positive.
 * Eval, envEval(dir): the texel and radiance are exactly envLookup's — the same normalize, atan2_WAR, det_acos and
 *   truncation (the device's conversion: NaN and negatives 0), zero outside the map; pdf is the formula above with
 *   st = sqrtf(max(0, 1 - pd.y * pd.y)), pd the normalised direction, evaluated as sqrtf(pd.x * pd.x + pd.z * pd.z): the
 *   same quantity without the cancellation, which below st = 0.03 would cost more than the 1e-4 by which the two pdfs may
 *   differ (a unit vector's y alone holds the polar angle only to sqrt(1e-7) near the poles).  Outside the map: radiance 0, pdf 0, texel 0xFFFFFFFF
 *   (u reaches 1 for directions with x = +0, z > 0).  A NaN or zero direction (its normalisation is NaN) looks up
 *   texel (W / 2, 0), as envLookup does: every comparison of atan2_WAR fails, so u = 0.5, and the NaN v converts to row 0;
 *   its pdf is 0.
 *
 * bdpt_env_prepare snapshots the map bound by bdpt_set_environment (the map stays caller memory and is read by every later
 * query; the table is the context's).  It needs a map: a constant colour or no environment gives BDPT_E_STATE.  It allocates
 * on first use and when the size changes, so that call must not be inside a stream capture (BDPT_E_STATE there), as the
 * emitter table's first build; a repeat call with the same size allocates nothing, does not synchronise and can be captured
 * (three kernel nodes): the re-prepare after an animated probe.  bdpt_set_environment and bdpt_destroy
 * drop the table: the calls below then return BDPT_E_STATE until bdpt_env_prepare ran again.  bdpt_get_env_info
 * synchronises (it reads total and m back).
 *
 * bdpt_env_query, per item i < min(*numDevice, num):
 *   BDPT_ENV_SAMPLE  in: surfaces[i], seeds[i]; out: samples[i] (five float4), seedsOut[i] (optional, may be `seeds`): the
 *     state after the four draws.  ray = (posW, minT, dir, 1e38); radiance, pdf, texel as above;
 *     value = the unweighted contribution of a visible environment, +0 when pdf == 0: with matIndex 1
 *       (((NdotL * radiance) * diffuse) / kPi) / pdf, NdotL = saturate(dot(N, dir)); with matIndex 0 the pass's GGX term
 *       directIfVisible(lightsCount 1, L = dir, intensity = radiance) / pdf — (D G F / (4 NdotV) + NdotL diffuse / kPi) times
 *       radiance, the device function next-event estimation runs.  Throughput, weight and clamp stay with the caller.
 *     status = BDPT_ENV_STATUS_NONZERO when value has a component that is not +-0.  A record with prim < 0 gives an
 *     all-zero sample and still takes its four draws.  With compactRays / compactItems / compactCount (all three, as
 *     bdpt_light_query) the rays of the NONZERO items go to a dense list for bdpt_trace_rays(BDPT_TRACE_ANY).
 *   BDPT_ENV_EVAL    in: dirs[i] (float4, xyz read); out: evals[i] (two float4): radiance, pdf, texel.
 * Record contract: posW, N, V, linearRoughness, diffuse, specular and prim (its sign) are read; floats may be degenerate or
 * not finite, the outputs are those of the fp32 arithmetic as written.  Nothing a caller supplies reaches an address: a
 * texel index comes only from the table search, bounded by W and H whatever the table holds, or from envLookup's
 * bounds-checked truncation.
 *
 * bdpt_sky_query: item i alive iff surfaces[i].prim >= 0 and (alive == NULL or alive[i] != 0).  For an alive item
 *   s = seeds[i]; sum = 0; count = 0
 *   for k = 0 .. samples-1 (1 .. BDPT_SKY_MAX_SAMPLES):
 *     (ray, radiance, pdf) = envSample(s)                                           four draws
 *     value = clampVec((((NdotL * radiance) * diffuse) / kPi) / pdf, clampUpper), +0 when pdf == 0
 *     term  = value when every component is +-0 (no ray is traced); else +0 when the ray is occluded as BDPT_TRACE_ANY
 *             answers it; else value, and count += 1
 *     sum += term                                                                   in k order
 *   color[i] = (sum / (float)samples, 1); counts[i] = count; seedsOut[i] = s
 * A dead item gets color = (diffuse.rgb, 1) — the G-buffer's environment colour on a miss, as bdpt_gi_query — counts 0 and
 * its seed unchanged: no draw.  This equals the composed loop bdpt_env_query(SAMPLE, matIndex 1) -> clamp ->
 * bdpt_trace_rays(ANY) on the non-zero terms -> ordered add, bit for bit.  Only posW, N, diffuse and prim are read.
 * bdpt_sky_execute runs the same for the context's tile pixels with the seed initRand(x + y * width, frameCount, 16), the
 * full-frame worldPosition, worldNormal and materialDiffuse channels, alive iff worldPosition.w != 0 — bdpt_gi_execute's
 * rules, so tiles reproduce the whole frame.  It needs a scene, a size and a prepared table, no camera.
 *
 * Ordering, capture, counters and numDevice: as bdpt_light_query and bdpt_ao_query (one kernel node per query).
 * Errors (nothing is enqueued), in this order: a NULL context, desc / params or gbuffer BDPT_E_INVALID; no scene
 * (bdpt_sky_*), no size (bdpt_sky_execute), no prepared table — none yet, or dropped by bdpt_set_environment — BDPT_E_STATE;
 * unknown mode or flags, matIndex > 1, samples outside 1 .. BDPT_SKY_MAX_SAMPLES, non-zero reserved, a partial compaction
 * triple, compaction with BDPT_ENV_EVAL BDPT_E_INVALID; then num == 0 returns BDPT_OK; then a missing or misaligned buffer
 * BDPT_E_INVALID: records and `out` 16 bytes, the half channels 8, words 4. */
#define BDPT_ENV_MAX_DIM 16384u
#define BDPT_ENV_SAMPLE 0u
#define BDPT_ENV_EVAL 1u
#define BDPT_ENV_STATUS_NONZERO 1u
#define BDPT_SKY_MAX_SAMPLES 64u
typedef struct bdpt_env_info {
  uint32_t width, height;
  uint64_t total;           /* rowCdf[H - 1] */
  float max;                /* m */
  uint32_t rowScanChunk;    /* texels per pass of the row scan */
  uint32_t marginalChunk;   /* rows per pass of the marginal scan */
  uint32_t reserved;
  uint64_t tableBytes;      /* device bytes the table holds */
  const uint32_t* cdf;      /* device addresses of the table (stable across a re-prepare of the same size) */
  const uint64_t* rowCdf;
} bdpt_env_info; /* 56 bytes */
int bdpt_env_prepare(bdpt_ctx* ctx, void* stream);
int bdpt_get_env_info(bdpt_ctx* ctx, bdpt_env_info* out); /* synchronises */
typedef struct bdpt_env_sample {
  bdpt_ray ray;       /* org = posW, tmin = minT, dir, tmax = 1e38 */
  float radiance[3];  /* the chosen texel's rgb */
  float pdf;          /* solid angle */
  float value[3];
  uint32_t texel;     /* y * W + x */
  uint32_t status;    /* BDPT_ENV_STATUS_NONZERO or 0 */
  uint32_t reserved[3];
} bdpt_env_sample; /* 80 bytes: five float4 */
typedef struct bdpt_env_eval {
  float radiance[3];
  float pdf;
  uint32_t texel;     /* 0xFFFFFFFF: outside the map */
  uint32_t reserved[3];
} bdpt_env_eval; /* 32 bytes: two float4 */
typedef struct bdpt_env_desc {
  uint32_t mode;                /* BDPT_ENV_SAMPLE or BDPT_ENV_EVAL */
  uint32_t num;                 /* items; the capacity when numDevice is set */
  const uint32_t* numDevice;    /* optional device word: min(*numDevice, num) items */
  uint32_t matIndex;            /* SAMPLE: 0 GGX, 1 Lambertian */
  uint32_t flags;               /* 0 */
  float minT;                   /* SAMPLE: tmin of the rays */
  uint32_t reserved;            /* 0 */
  const bdpt_surface* surfaces; /* SAMPLE: device, 16-byte aligned, num records */
  const uint32_t* seeds;        /* SAMPLE: device, num RNG states */
  uint32_t* seedsOut;           /* SAMPLE, optional: device, num RNG states (may be `seeds`) */
  bdpt_env_sample* samples;     /* SAMPLE: device, 16-byte aligned, num records */
  const float* dirs;            /* EVAL: device, 16-byte aligned, num float4 (xyz read) */
  bdpt_env_eval* evals;         /* EVAL: device, 16-byte aligned, num records */
  bdpt_ray* compactRays;        /* SAMPLE, optional, all three or none: as bdpt_light_desc */
  uint32_t* compactItems;
  uint32_t* compactCount;
} bdpt_env_desc;
int bdpt_env_query(bdpt_ctx* ctx, const bdpt_env_desc* desc, void* stream);
typedef struct bdpt_sky_desc {
  uint32_t num;                 /* items; the capacity when numDevice is set */
  uint32_t samples;             /* 1 .. BDPT_SKY_MAX_SAMPLES */
  const uint32_t* numDevice;    /* optional device word: min(*numDevice, num) items */
  float clampUpper;             /* upper bound of every component of a sample's value (clampVec) */
  float minT;                   /* tmin of the rays */
  uint32_t flags;               /* 0 */
  uint32_t reserved;            /* 0 */
  const bdpt_surface* surfaces; /* device, 16-byte aligned, num records: posW, N, diffuse and prim are read */
  const uint32_t* seeds;        /* device, num RNG states */
  const uint8_t* alive;         /* optional: device, one byte per item, 0 = the item is dead */
  float* color;                 /* device, 16-byte aligned, num float4 */
  uint32_t* counts;             /* optional: device, num words: the samples traced and found unoccluded */
  uint32_t* seedsOut;           /* optional: device, num RNG states (may be `seeds`) */
} bdpt_sky_desc;
int bdpt_sky_query(bdpt_ctx* ctx, const bdpt_sky_desc* desc, void* stream);
typedef struct bdpt_sky_params {
  uint32_t frameCount;
  float clampUpper;
  float minT;
  uint32_t samples;  /* 1 .. BDPT_SKY_MAX_SAMPLES */
  uint32_t reserved; /* 0 */
} bdpt_sky_params;
int bdpt_sky_execute(bdpt_ctx* ctx, const bdpt_sky_params* p, const bdpt_gbuffer* gbuffer, float* out, void* stream);
/* MIS sky lighting: the BSDF's density toward a given direction, and the fused pass with table samples and BSDF samples
 * combined by the balance heuristic, for the pass's GGX material or the Lambertian one.  bdpt_sky_query above stays as it is.
 *
 * bdpt_bsdf_pdf_query, per item i < min(*numDevice, num): in surfaces[i], dirs[i] (float4, xyz = L, used as given);
 * out values[i] = (fcos.xyz, pdf): fcos the unweighted BSDF times cosine that next-event estimation uses, pdf the
 * solid-angle density with which bdpt_bsdf_query(BDPT_BSDF_SAMPLE) draws L; rough = linearRoughness^2 as there.  Built from
 * the pass's device functions, fp32 as written, without contraction:
 *   matIndex 1: NdotL = saturate(dot(N, L)); fcos = (NdotL * diffuse) / kPi; pdf = NdotL * kInvPi (sampleBRDF's expression)
 *   matIndex 0: fcos = directIfVisible(lightsCount 1, L, intensity (1, 1, 1)) = D G F / (4 NdotV) + NdotL diffuse / kPi;
 *               pdf = 0 when dot(N, L) <= 0, otherwise pdfD + pdfS with pd = probabilityToSampleDiffuse(diffuse, specular),
 *               pdfD = (NdotL * kInvPi) * pd, H = normalize(V + L), NdotH = saturate(dot(N, H)), LdotH = saturate(dot(L, H)),
 *               pdfS = (ggxNormalDistribution(NdotH, rough) * NdotH / (4 * LdotH)) * (1.0f - pd): the one-sample mixture of
 *               sampleBRDF's two lobes.
 * A record with prim < 0 gives zeros.  numDevice, stream ordering, capture (one kernel node), the error order and the
 * record contract are bdpt_bsdf_query's: N, V, linearRoughness, diffuse, specular and prim (its sign) are read, floats may be
 * degenerate or not finite, the outputs are those of the fp32 arithmetic as written, nothing a caller supplies reaches an
 * address.  flags and reserved must be 0.
 *
 * bdpt_sky_mis_query: item i alive as for bdpt_sky_query.  techniques: bit 0 table samples, bit 1 BSDF samples (1, 2 or 3).
 * For an alive item
 *   s = seeds[i]; sum = 0; count = 0
 *   for k = 0 .. samples-1 (1 .. BDPT_SKY_MAX_SAMPLES):
 *     bit 0 set, the table-sampled term L_k:
 *       e = envSample(s)                                                              four draws
 *       (fcos, pB) = the function above toward e.dir; with bit 1 clear pB counts as +0
 *       termL = e.pdf == 0 ? +0 : clampVec((fcos * e.radiance) / (e.pdf + pB), clampUpper)
 *     bit 1 set, the BSDF-sampled term B_k:
 *       b = sampleBRDF(s by value, N, N, V, ...): what bdpt_bsdf_query(BDPT_BSDF_SAMPLE, flags 0) returns for state s;
 *       then s advances by exactly three draws, for either material (the samplers take two or three)
 *       ev = envEval(b.dir); (fcos, pB) toward b.dir; with bit 0 clear ev.pdf counts as +0
 *       termB = b.pdf == 0 ? +0 : clampVec((fcos * ev.radiance) / (ev.pdf + pB), clampUpper)
 *     each term, in the order L_0, B_0, L_1, B_1, ...: all +-0: added at once, no ray is traced; else the ray
 *       (posW, minT, dir, 1e38) is traced as BDPT_TRACE_ANY traces it: occluded adds +0, unoccluded adds the term and
 *       count += 1
 *   color[i] = (sum / (float)samples, 1); counts[i] = count, 0 .. 2 * samples; seedsOut[i] = s after 4, 3 or 7 draws a sample
 * A dead item is handled as by bdpt_sky_query.  This is the balance heuristic with one sample per technique; with one
 * technique it is the plain estimator, so techniques 1 with matIndex 0 is the GGX variant of bdpt_sky_query.  The call
 * equals the composed loop bdpt_env_query(SAMPLE) -> bdpt_bsdf_pdf_query -> bdpt_bsdf_query(SAMPLE) -> bdpt_env_query(EVAL)
 * -> bdpt_bsdf_pdf_query -> elementwise fp32 arithmetic -> bdpt_trace_rays(ANY) twice -> ordered adds, bit for bit.
 * bdpt_sky_mis_execute runs the same for the context's tile pixels: seeds initRand(x + y * width, frameCount, 16); the
 * full-frame worldPosition, worldNormal and materialDiffuse, and for matIndex 0 materialSpecRough (specular = rgb, rough =
 * a * a) with V = normalize(camera position - posW), as the frame's first vertex; alive iff worldPosition.w != 0.  Tiles
 * and stripes reproduce the whole frame.
 * Errors, in this order: a NULL context, desc / params or gbuffer BDPT_E_INVALID; no scene, no size (execute), no prepared
 * table, no camera (execute with matIndex 0) BDPT_E_STATE; samples outside 1 .. BDPT_SKY_MAX_SAMPLES, matIndex > 1,
 * techniques outside 1 .. 3, non-zero flags or reserved BDPT_E_INVALID; then num == 0 returns BDPT_OK; then a missing or
 * misaligned buffer BDPT_E_INVALID. */
#define BDPT_SKY_MIS_TABLE 1u
#define BDPT_SKY_MIS_BSDF 2u
typedef struct bdpt_bsdf_pdf_desc {
  uint32_t num;                 /* items; the capacity when numDevice is set */
  uint32_t matIndex;            /* 0 GGX, 1 Lambertian */
  const uint32_t* numDevice;    /* optional device word: min(*numDevice, num) items */
  uint32_t flags;               /* 0 */
  uint32_t reserved;            /* 0 */
  const bdpt_surface* surfaces; /* device, 16-byte aligned, num records */
  const float* dirs;            /* device, 16-byte aligned, num float4 (xyz = L) */
  float* values;                /* device, 16-byte aligned, num float4: (fcos, pdf) */
} bdpt_bsdf_pdf_desc; /* 48 bytes */
int bdpt_bsdf_pdf_query(bdpt_ctx* ctx, const bdpt_bsdf_pdf_desc* desc, void* stream);
typedef struct bdpt_sky_mis_desc {
  uint32_t num;                 /* items; the capacity when numDevice is set */
  uint32_t samples;             /* 1 .. BDPT_SKY_MAX_SAMPLES */
  const uint32_t* numDevice;    /* optional device word: min(*numDevice, num) items */
  float clampUpper;             /* upper bound of every component of a term (clampVec) */
  float minT;                   /* tmin of the rays */
  uint32_t matIndex;            /* 0 GGX, 1 Lambertian */
  uint32_t techniques;          /* BDPT_SKY_MIS_TABLE | BDPT_SKY_MIS_BSDF: 1, 2 or 3 */
  uint32_t flags;               /* 0 */
  uint32_t reserved;            /* 0 */
  const bdpt_surface* surfaces; /* device, 16-byte aligned, num records */
  const uint32_t* seeds;        /* device, num RNG states */
  const uint8_t* alive;         /* optional: device, one byte per item, 0 = the item is dead */
  float* color;                 /* device, 16-byte aligned, num float4 */
  uint32_t* counts;             /* optional: device, num words: the terms traced and found unoccluded */
  uint32_t* seedsOut;           /* optional: device, num RNG states (may be `seeds`) */
} bdpt_sky_mis_desc; /* 88 bytes */
int bdpt_sky_mis_query(bdpt_ctx* ctx, const bdpt_sky_mis_desc* desc, void* stream);
typedef struct bdpt_sky_mis_params {
  uint32_t frameCount;
  float clampUpper;
  float minT;
  uint32_t samples;     /* 1 .. BDPT_SKY_MAX_SAMPLES */
  uint32_t matIndex;    /* 0 GGX (needs a camera), 1 Lambertian */
  uint32_t techniques;  /* 1, 2 or 3 */
  uint32_t reserved[2]; /* 0 */
} bdpt_sky_mis_params; /* 32 bytes */
int bdpt_sky_mis_execute(bdpt_ctx* ctx, const bdpt_sky_mis_params* p, const bdpt_gbuffer* gbuffer, float* out, void* stream);
/* Host twins (no GPU, no context): csrc/env_light.h on the CPU.  bdpt_host_env_table fills q (optional), cdf (W * H words),
 * rowCdf (H words) and *outMax (optional) for a host map; BDPT_E_LIMIT past BDPT_ENV_MAX_DIM.  bdpt_host_env_sample runs
 * envSample for n states (seedsOut optional, may be `seeds`); bdpt_host_env_eval runs envEval for n float4 directions. */
typedef struct bdpt_env_host_sample {
  float dir[3];
  float pdf;
  float radiance[3];
  uint32_t texel;
} bdpt_env_host_sample; /* 32 bytes */
int bdpt_host_env_table(const float* map, uint32_t width, uint32_t height, uint32_t* q, uint32_t* cdf, uint64_t* rowCdf, float* outMax);
int bdpt_host_env_sample(const float* map, uint32_t width, uint32_t height, const uint32_t* cdf, const uint64_t* rowCdf,
                         const uint32_t* seeds, uint32_t n, bdpt_env_host_sample* out, uint32_t* seedsOut);
int bdpt_host_env_eval(const float* map, uint32_t width, uint32_t height, const uint32_t* cdf, const uint64_t* rowCdf, const float* dirs,
                       uint32_t n, bdpt_env_eval* out);
/* Test hook: the context's table read back to host memory (cdf: W * H words, rowCdf: H words); synchronises. */
int bdpt_test_env_table(bdpt_ctx* ctx, uint32_t* cdf, uint64_t* rowCdf);
/* Host-only test hook: the table search of envSample (csrc/env_light.h envSearch) for n pairs of draws given directly, so
 * that a test can aim at every boundary of both tables (through seeds the second draw is a function of the first):
 * texels[i] = y * W + x for draws r1[i], r2[i] in [0, 1) (any other value, a NaN included: BDPT_E_INVALID, nothing is
 * written).  BDPT_E_STATE when the tables' total is 0. */
int bdpt_test_host_env_search(uint32_t width, uint32_t height, const uint32_t* cdf, const uint64_t* rowCdf, const float* r1, const float* r2,
                              uint32_t n, uint32_t* texels);

/* ---- Resampled direct lighting -------------------------------------------------------------------------------------
 * Direct lighting with one any-hit ray per item and sample whatever the light count: resampled importance sampling (RIS),
 * the first stage of ReSTIR.  Per sample `candidates` (M) next-event samples of the pass are drawn, one of them is kept in
 * a one-entry reservoir with probability proportional to its unshadowed, clamped contribution at the item, and one ray is
 * traced for the survivor; `samples` (K) such estimates are averaged.  The emitter table (BDPT_PARAM_AREA_LIGHTS) is one
 * more candidate source.  bdpt_direct_query is the converged answer for the scene's lights (without the pass's clamp and
 * with its own albedo rule); this estimates the clamped next-event term of the pass.
 *
 * bdpt_ris_query: item i < min(*numDevice, num) is dead when alive[i] == 0 or surfaces[i].prim < 0.  A dead item takes no
 * draw: color[i] = (diffuse, 1), traced[i] = 0, seedsOut[i] = seeds[i], its reservoirs are "no selection" records with
 * wsum = +0 (what bdpt_sky_mis_query gives a dead item).  For an alive item
 *   s = seeds[i]; sum = 0
 *   lightsCount as bdpt_light_query has it: numLights, plus one for the table with BDPT_PARAM_AREA_LIGHTS while its W > 0
 *   for k = 0 .. samples-1:
 *     wsum = 0; nothing selected
 *     for c = 0 .. candidates-1:
 *       (ray_c, value_c, light_c) = what bdpt_light_query(BDPT_LIGHT_NEE, matIndex, flags & BDPT_PARAM_AREA_LIGHTS) returns
 *         for state s: one draw, s advances once; state_c = s after that draw (the state areaNee forks its three uniforms
 *         from).  No hint is tried for a candidate.
 *       u_c = nextRand(s)                                    always taken
 *       v_c = clampVec(value_c, clampUpper)                  NaN and negative components become +0
 *       w_c = max(max(v_c.x, v_c.y), v_c.z)                  max(a, b) = b > a ? b : a; never NaN, >= 0
 *       wsum = wsum + w_c
 *       candidate c becomes the selection iff w_c > 0 && u_c * wsum <= w_c      (<=: the first positive one is always taken)
 *     nothing selected: the sample's term is +0, no ray
 *     otherwise W = (wsum / (float)candidates) / w_sel; term = v_sel * W
 *       with BDPT_RIS_USE_HINTS, a selected point or spot light whose term has a positive component first tries the light's
 *         occluder hint, the test bdpt_light_query makes (BDPT_LIGHT_USE_HINTS): occluded, the term counts as +0, no ray
 *       otherwise ray_sel = (posW, minT, L, distance as bdpt_light_query gives it) is traced as BDPT_TRACE_ANY traces it;
 *         occluded, the term counts as +0
 *     sum = sum + term
 *   color[i] = (sum / (float)samples, 1); seedsOut[i] = s after 2 * candidates * samples draws; traced[i] = rays traversed
 * Every operation is one fp32 rounding in the order written, without contraction.  The record contract of "Light queries"
 * applies unchanged: degenerate and non-finite records give what this arithmetic gives, nothing a caller supplies reaches
 * an address.  With candidates = 1, W is exactly 1 for a finite positive weight and the call is plain next-event
 * estimation: bdpt_light_query -> bdpt_trace_rays(ANY) -> mask.  The estimator is unbiased for the clamped direct
 * lighting: the candidates come from one source density whose reciprocal is already inside `value`.
 * reservoirs (optional): samples records per item, record k of item i at [i * samples + k].  No selection: light 0xffff,
 * status 0, state 0, W = +0.  status: BDPT_RIS_STATUS_RAY a ray was needed (something was selected),
 * BDPT_RIS_STATUS_HINT_OCCLUDED the hint answered it, BDPT_RIS_STATUS_OCCLUDED the traced ray was occluded.  `light` and
 * `state` reproduce the sampled point for any receiver: getLightData serves a light, areaNee(state) the table
 * (light == numLights) — what a later reuse stage needs.
 * bdpt_ris_execute runs the same for the context's tile pixels: seeds initRand(x + y * width, frameCount, 16); the
 * full-frame worldPosition, worldNormal and materialDiffuse, and for matIndex 0 materialSpecRough (specular = rgb, rough =
 * a * a) with V = normalize(camera position - posW); alive iff worldPosition.w != 0, a background pixel gets (diffuse, 1).
 * Tiles and stripes reproduce the whole frame.
 * Both calls are stream-ordered, capturable (one kernel node) and allocate nothing, but for the emitter table, which
 * follows bdpt_light_query's rule: bdpt_prepare(BDPT_PREPARE_AREA_LIGHTS) makes it, or the first call that needs it does;
 * that first call inside a capture returns BDPT_E_STATE.
 * Errors, in this order: a NULL context, desc / params or gbuffer BDPT_E_INVALID; no scene, no size (execute), no camera
 * (execute with matIndex 0) BDPT_E_STATE; candidates outside 1 .. BDPT_RIS_MAX_CANDIDATES, samples outside 1 ..
 * BDPT_RIS_MAX_SAMPLES, matIndex > 1, an unknown flag, non-zero reserved, a negative or NaN clampUpper BDPT_E_INVALID;
 * then num == 0 returns BDPT_OK; then a missing or misaligned buffer BDPT_E_INVALID.  A refused call enqueues nothing. */
#define BDPT_RIS_USE_HINTS 1u /* flags, beside BDPT_PARAM_AREA_LIGHTS */
#define BDPT_RIS_MAX_CANDIDATES 32u
#define BDPT_RIS_MAX_SAMPLES 64u
#define BDPT_RIS_STATUS_RAY 1u
#define BDPT_RIS_STATUS_HINT_OCCLUDED 2u
#define BDPT_RIS_STATUS_OCCLUDED 4u
#define BDPT_RIS_NO_LIGHT 0xffffu
typedef struct bdpt_ris_reservoir {
  uint16_t light;  /* the selected light (numLights = the emitter table), BDPT_RIS_NO_LIGHT when nothing was selected */
  uint16_t status; /* BDPT_RIS_STATUS_* */
  uint32_t state;  /* the RNG state after the selection draw of the selected candidate */
  float W;         /* (wsum / candidates) / w_sel */
  float wsum;
} bdpt_ris_reservoir; /* 16 bytes */
typedef struct bdpt_ris_desc {
  uint32_t num;                 /* items; the capacity when numDevice is set */
  uint32_t flags;               /* BDPT_PARAM_AREA_LIGHTS | BDPT_RIS_USE_HINTS */
  const uint32_t* numDevice;    /* optional device word: min(*numDevice, num) items */
  uint32_t matIndex;            /* 0 GGX, 1 Lambertian */
  uint32_t candidates;          /* 1 .. BDPT_RIS_MAX_CANDIDATES */
  uint32_t samples;             /* 1 .. BDPT_RIS_MAX_SAMPLES */
  float clampUpper;             /* upper bound of every component of a candidate's value (clampVec); >= 0 */
  float minT;                   /* tmin of the rays and of the hint test */
  uint32_t reserved;            /* 0 */
  const bdpt_surface* surfaces; /* device, 16-byte aligned, num records */
  const uint8_t* alive;         /* optional: device, one byte per item, 0 = the item is dead */
  const uint32_t* seeds;        /* device, num RNG states */
  float* color;                 /* device, 16-byte aligned, num float4 */
  uint32_t* seedsOut;           /* optional: device, num RNG states (may be `seeds`) */
  uint32_t* traced;             /* optional: device, num words: the rays traversed */
  bdpt_ris_reservoir* reservoirs; /* optional: device, 16-byte aligned, num * samples records */
} bdpt_ris_desc; /* 96 bytes */
int bdpt_ris_query(bdpt_ctx* ctx, const bdpt_ris_desc* desc, void* stream);
typedef struct bdpt_ris_params {
  uint32_t frameCount;
  float clampUpper;
  float minT;
  uint32_t candidates; /* 1 .. BDPT_RIS_MAX_CANDIDATES */
  uint32_t samples;    /* 1 .. BDPT_RIS_MAX_SAMPLES */
  uint32_t matIndex;   /* 0 GGX (needs a camera), 1 Lambertian */
  uint32_t flags;      /* BDPT_PARAM_AREA_LIGHTS | BDPT_RIS_USE_HINTS */
  uint32_t reserved;   /* 0 */
} bdpt_ris_params; /* 32 bytes */
int bdpt_ris_execute(bdpt_ctx* ctx, const bdpt_ris_params* p, const bdpt_gbuffer* gbuffer, float* out, void* stream);

/* ---- Reservoir reuse -----------------------------------------------------------------------------------------------
 * The second stage of ReSTIR: an item combines its own reservoir with those of up to BDPT_REUSE_MAX_NEIGHBORS other
 * surface points (spatial neighbours, or the same point a frame ago) and traces ONE any-hit ray for the survivor.  It is
 * the unbiased 1 / Z combination of Bitterli et al. 2020, Algorithm 6.  The target is the unshadowed, clamped value, as in
 * the first stage; visibility is not reused (the OCCLUDED bits of input records are ignored), so the result is unbiased
 * for the clamped direct lighting, bdpt_ris_query's own contract.
 *
 * A reservoir's sample can be re-evaluated at any receiver.  A record's `state` is the RNG state after the selection draw
 * that chose `light`, and the generator is invertible: prev(s) = (s - 1013904223) * 4276115653 mod 2^32.
 * bdpt_light_query(BDPT_LIGHT_NEE) from prev(state) at any surface record draws the same light, and for the emitter table
 * the same emitter point (areaNee forks from `state`; its point does not depend on the receiver).  The composed loop is
 * prev(state) -> bdpt_light_query -> clamp; the kernel evaluates (light, state) directly.  `light` must be the light that
 * prev(state) draws, as it is in every record bdpt_ris_query and this call write; for any other in-range `light` the
 * value is that light's.
 *
 * bdpt_reuse_query: item i < min(*numDevice, num) is dead as bdpt_ris_query has it.  A dead item gets color (diffuse, 1),
 * no draw (seedsOut[i] = seeds[i]), traced 0 and the empty record (BDPT_RIS_NO_LIGHT, 0, 0, +0, M = 0).  For an alive
 * item the sources are, in order, its own record in[i] at surface i, then for n = 0 .. neighbors-1 the pool entry
 * p_n = neighborIndex[i * neighbors + n] with record pool[p_n] at surface poolSurfaces[p_n].  A neighbour slot is skipped
 * (its draw is still taken) when p_n >= poolNum (0xffffffff is the conventional "none"), when the pool item is dead (by
 * poolAlive and prim, the items' rule), when !(dot(N_i, N_p) >= normalMin), or when
 * !(fabsf(dot(N_i, pos_p - pos_i)) <= planeMax); dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z.
 * Candidate counts: a record's count is inM (for in) / poolM (for pool) when that scalar is non-zero — how first-stage
 * bdpt_ris_reservoir records are read, whose fourth word is wsum — and the record's M word otherwise; counts above
 * BDPT_REUSE_MAX_M read as that; pool counts are then capped by maxM, the own count is not.
 *   t_x(y), v_x(y): v = clampVec(value of sample y at surface x, clampUpper), t = max(max(v.x, v.y), v.z)
 *                   value as bdpt_light_query(NEE, matIndex, flags & BDPT_PARAM_AREA_LIGHTS) gives it; y.light >=
 *                   lightsCount or == BDPT_RIS_NO_LIGHT, or !(y.W > 0): the record is empty, w = 0
 *   s = seeds[i]; wsum = 0; Mtot = 0 (uint32)
 *   for each source j in order:  u_j = nextRand(s)            always taken, 1 + neighbors draws per item
 *       skipped slot: continue
 *       w = (t_i(y_j) * W_j) * (float)M_j;  wsum = wsum + w;  Mtot += M_j
 *       source j becomes the selection iff w > 0 && u_j * wsum <= w
 *   nothing selected: colour term +0, no ray, out = (BDPT_RIS_NO_LIGHT, status 0, state 0, W +0, Mtot)
 *   Z = sum of M_j over the non-skipped sources with t_j(y_sel) > 0      (t at source j's own surface, the same material)
 *   Z == 0: as nothing selected
 *   W' = (wsum / (float)Z) / t_i(y_sel);  term = v_i(y_sel) * W'
 *   one BDPT_TRACE_ANY ray (pos_i, minT, L, distance as bdpt_light_query gives them for y_sel at i); occluded: +0
 *   color[i] = (term or +0, 1); out[i] = (light, status, state, W', Mtot) with status BDPT_RIS_STATUS_RAY, and
 *   BDPT_RIS_STATUS_OCCLUDED when so; traced[i] = 1; seedsOut[i] = s after 1 + neighbors draws
 * Every operation is one fp32 rounding in the order written, without contraction.  Nothing a caller supplies reaches an
 * address: neighbour indices, light ids and counts are range-checked as above.  No occluder hints in this stage.
 * The pool may be the item arrays themselves (spatial reuse) or another set (last frame's: temporal reuse).  Not enforced:
 * temporal reuse assumes that the lights and the emitter table are those the history was made with, and the states that
 * made the input reservoirs must be independent of `seeds`.
 * The call is stream-ordered, capturable (one kernel node) and allocates nothing but the emitter table, under
 * bdpt_ris_query's rule.  Errors, in this order: a NULL context or desc BDPT_E_INVALID; no scene BDPT_E_STATE; neighbors >
 * BDPT_REUSE_MAX_NEIGHBORS, matIndex > 1, a flag other than BDPT_PARAM_AREA_LIGHTS, non-zero reserved, a negative or NaN
 * clampUpper BDPT_E_INVALID; then num == 0 returns BDPT_OK; then a missing or misaligned buffer (neighborIndex with
 * neighbors > 0, poolSurfaces and pool with neighbors > 0 and poolNum > 0), or `out` equal to `in` or `pool`,
 * BDPT_E_INVALID.  A refused call enqueues nothing. */
#define BDPT_REUSE_MAX_NEIGHBORS 8u
#define BDPT_REUSE_MAX_M (1u << 24)
typedef struct bdpt_reuse_reservoir {
  uint16_t light;  /* as bdpt_ris_reservoir */
  uint16_t status; /* BDPT_RIS_STATUS_* */
  uint32_t state;  /* the RNG state after the selection draw that chose `light` */
  float W;
  uint32_t M;      /* the candidates the record stands for */
} bdpt_reuse_reservoir; /* 16 bytes */
typedef struct bdpt_reuse_desc {
  uint32_t num;              /* items; the capacity when numDevice is set */
  uint32_t flags;            /* BDPT_PARAM_AREA_LIGHTS */
  const uint32_t* numDevice; /* optional device word: min(*numDevice, num) items */
  uint32_t matIndex;         /* 0 GGX, 1 Lambertian */
  uint32_t neighbors;        /* 0 .. BDPT_REUSE_MAX_NEIGHBORS */
  uint32_t inM;              /* non-zero: the count of every `in` record */
  uint32_t poolM;            /* non-zero: the count of every `pool` record */
  uint32_t maxM;             /* cap of a pool record's count */
  uint32_t poolNum;          /* pool entries */
  float normalMin;           /* a neighbour needs dot(N_i, N_p) >= normalMin */
  float planeMax;            /* ... and fabsf(dot(N_i, pos_p - pos_i)) <= planeMax */
  float clampUpper;          /* as bdpt_ris_desc */
  float minT;                /* tmin of the ray */
  uint32_t reserved[2];      /* 0 */
  const bdpt_surface* surfaces;       /* device, 16-byte aligned, num records */
  const uint8_t* alive;               /* optional: device, one byte per item */
  const uint32_t* seeds;              /* device, num RNG states */
  const bdpt_reuse_reservoir* in;     /* device, 16-byte aligned, num records */
  const bdpt_surface* poolSurfaces;   /* device, 16-byte aligned, poolNum records (may be `surfaces`) */
  const uint8_t* poolAlive;           /* optional: device, one byte per pool entry */
  const bdpt_reuse_reservoir* pool;   /* device, 16-byte aligned, poolNum records (may be `in`) */
  const uint32_t* neighborIndex;      /* device, num * neighbors pool indices */
  float* color;                       /* device, 16-byte aligned, num float4 */
  uint32_t* seedsOut;                 /* optional: device, num RNG states (may be `seeds`) */
  uint32_t* traced;                   /* optional: device, num words: 1 where a ray was traversed */
  bdpt_reuse_reservoir* out;          /* optional: device, 16-byte aligned, num records; not `in`, not `pool` */
} bdpt_reuse_desc; /* 160 bytes */
int bdpt_reuse_query(bdpt_ctx* ctx, const bdpt_reuse_desc* desc, void* stream);
/* bdpt_reuse_execute runs the same for the context's tile pixels.  Items: the pixels of `gbuffer` as bdpt_ris_execute reads
 * them, with own records in[pixel] of a full-frame image.  Pool: the width * height pixels of poolGbuffer (it may be
 * `gbuffer`, or last frame's copy) with records pool[pixel]; a pool pixel is dead where its worldPosition.w is 0, and for
 * matIndex 0 its V is normalize(poolCameraPos - posW).  Seeds: initRand(initRand(pixel, frameCount), 0x52455553), the fork
 * idiom of the emitter table's stream, so a caller may reuse the frame counter of bdpt_ris_execute.  Colour and `out`
 * records are written at the tile's pixels only; two row tiles over a full-frame pool reproduce the frame.
 * Neighbours come from exactly one of three sources:
 *   neighborIndex set: a full-frame image, slot n of pixel p at [p * neighbors + n], of pool pixels
 *   BDPT_REUSE_SAME_PIXEL (neighbors must be 1): slot 0 is the pool pixel with the item's own index — the temporal pass
 *   otherwise (radius 1 .. BDPT_REUSE_MAX_RADIUS): before the selection draws each slot n = 0 .. neighbors-1 draws u1, u2;
 *     dx = (int)(u1 * (float)(2 * radius + 1)) - radius, dy likewise from u2; the slot is none when (dx, dy) == (0, 0) or
 *     (x + dx, y + dy) is outside the frame, else pool pixel (y + dy) * width + (x + dx).  The state after the 2 *
 *     neighbors draws is the s of the algorithm above.
 * Errors, in this order: a NULL context, params or gbuffer BDPT_E_INVALID; no scene, no size, no camera (matIndex 0)
 * BDPT_E_STATE; the scalar refusals of bdpt_reuse_query, an unknown flag, neighborIndex together with
 * BDPT_REUSE_SAME_PIXEL, BDPT_REUSE_SAME_PIXEL with neighbors != 1, or drawn offsets (neighbors > 0 and neither) with a
 * radius outside 1 .. BDPT_REUSE_MAX_RADIUS BDPT_E_INVALID; then a missing or misaligned buffer (the pool's with neighbors
 * > 0), or outReservoirs equal to `in` or `pool`, BDPT_E_INVALID. */
#define BDPT_REUSE_SAME_PIXEL 1u /* flags, beside BDPT_PARAM_AREA_LIGHTS */
#define BDPT_REUSE_MAX_RADIUS 1024u
typedef struct bdpt_reuse_params {
  uint32_t frameCount;
  float clampUpper;
  float minT;
  uint32_t matIndex;       /* 0 GGX (needs a camera), 1 Lambertian */
  uint32_t flags;          /* BDPT_PARAM_AREA_LIGHTS | BDPT_REUSE_SAME_PIXEL */
  uint32_t neighbors;      /* 0 .. BDPT_REUSE_MAX_NEIGHBORS */
  uint32_t radius;         /* drawn offsets: 1 .. BDPT_REUSE_MAX_RADIUS */
  uint32_t inM;            /* as bdpt_reuse_desc */
  uint32_t poolM;
  uint32_t maxM;
  float normalMin;
  float planeMax;
  float poolCameraPos[3];  /* V of pool pixels (matIndex 0) */
  uint32_t reserved;       /* 0 */
  const bdpt_reuse_reservoir* in;      /* device, 16-byte aligned, width * height records */
  const bdpt_gbuffer* poolGbuffer;     /* host: the pool's full-frame G-buffer (worldPosition, worldNormal, materialDiffuse,
                                          and for matIndex 0 materialSpecRough) */
  const bdpt_reuse_reservoir* pool;    /* device, 16-byte aligned, width * height records (may be `in`) */
  const uint32_t* neighborIndex;       /* optional: device, width * height * neighbors pool pixels */
  bdpt_reuse_reservoir* outReservoirs; /* optional: device, 16-byte aligned, width * height records; not `in`, not `pool` */
} bdpt_reuse_params; /* 104 bytes */
int bdpt_reuse_execute(bdpt_ctx* ctx, const bdpt_reuse_params* p, const bdpt_gbuffer* gbuffer, float* out, void* stream);
/* bdpt_ris_execute with a full-frame reservoir image: width * height * samples records, record k of pixel p at
 * [p * samples + k], written at the tile's pixels that are geometry; a background pixel's records are left as they are
 * (bdpt_reuse_execute reads the record of no background pixel, item or pool).  `out` is what bdpt_ris_execute writes,
 * bit for bit.  reservoirs missing or not 16-byte aligned: BDPT_E_INVALID, with the buffers. */
int bdpt_ris_execute_reservoirs(bdpt_ctx* ctx, const bdpt_ris_params* p, const bdpt_gbuffer* gbuffer, float* out,
                                bdpt_ris_reservoir* reservoirs, void* stream);

/* Host-only (no GPU, no context): run the acceleration-structure builder on a scene (geometry only: every triangle
 * opaque) and check its invariants — every triangle referenced, every leaf entry in exactly one leaf, the pieces of
 * a split triangle covering it, every child box containing its subtree's pieces, depth within the traversal stack.
 * Returns BDPT_OK and fills *out, or BDPT_E_INVALID with the first violated invariant in msg (msgCap bytes, may be NULL). */
int bdpt_bvh_build_check(const bdpt_scene_desc* scene, bdpt_bvh_info* out, char* msg, uint32_t msgCap);

/* Host-only test hook: build with `threads` host threads (0 = default: BDPT_BUILD_THREADS, else the CPUs this
 * process may use) and return a 64-bit FNV-1a hash of the node array, the leaf-ordered triangle list and the
 * summary; the tree must not depend on the thread count.  A scene with materials is built exactly as bdpt_set_scene
 * builds it (traversal flags, alpha classification, pre-splitting), one without as plain geometry.  out_info may be
 * NULL (its `reserved` field returns the default thread count). */
int bdpt_bvh_build_hash(const bdpt_scene_desc* scene, int threads, uint64_t* out_hash, bdpt_bvh_info* out_info);

/* Test hook: the builder the host-only hooks above and below use for the BINARY TREE stage — device >= 0: the device
 * implementation bdpt_set_scene uses (csrc/bvh_device.hip) on that device; device < 0: the host code (the default).  The
 * two build the same tree bit for bit; the GPU tests compare bdpt_bvh_build_hash under both settings. */
int bdpt_test_tree_builder(int device);
/* Test hook: FNV-1a over the packed records (every node, every leaf triangle) and the summary of a scene's acceleration
 * structure.  device < 0: everything by the host code; device >= 0: as bdpt_set_scene builds it — classification and split
 * priorities, references, binary tree, four-wide collapse, quantisation and packing on that device — with the records read back.  The two must agree; info->reserved = number of records. */
int bdpt_bvh_recs_hash(const bdpt_scene_desc* scene, int device, uint64_t* out_hash, bdpt_bvh_info* out_info);

/* Host-only test hooks: the acceleration structure exactly as bdpt_set_scene builds it (traversal flags, alpha
 * classification, spatial pre-splitting; negative budgets = build defaults, classify = 0 keeps the reference's
 * per-material opacity) walked on the CPU with the device's query semantics (bdpt_test_trace), or — brute != 0 —
 * the linear scan over every input triangle with the reference's per-material flags, which defines the right
 * answer.  rays: n x 8 floats (origin, direction, tmin, tmax); out_visits[2] = interior-node visits and triangle
 * tests summed over the rays (tree walk only).  The scene description must outlive the handle. */
void* bdpt_host_bvh_create(const bdpt_scene_desc* scene, int threads, float splitBudget, float splitBudgetAlpha, int classify,
                           bdpt_bvh_info* out_info);
void bdpt_host_bvh_destroy(void* handle);
int bdpt_host_bvh_trace(void* handle, const float* rays, uint32_t n, int mode, int brute, int threads, int32_t* out_prim,
                        float* out_tuv, uint64_t* out_visits);
/* Host-only test hooks of the refit (bdpt_update_geometry): refit the handle's tree to new positions (numVertices x 3
 * host floats) with the host refit, which the device refit matches bit for bit; bdpt_host_bvh_trace then walks the
 * refitted tree and its brute-force scan uses the new positions.  _refit_check: every record still reached as built,
 * words 10-11 and the leaf bits of every node and prim / flags / aux of every triangle unchanged, every triangle inside
 * every decoded ancestor box (BDPT_E_INVALID + msg otherwise).  _recs_hash: FNV-1a over the handle's records (as
 * bdpt_bvh_recs_hash); bdpt_ctx_recs_hash: the same over a context's records (synchronises).  _refit_info: as
 * bdpt_get_refit_info.  _refit_pieces: derives the piece regions of the handle's tree as built
 * (BDPT_PREPARE_REFIT_PIECES on the host) and makes later _refit calls use them; BDPT_E_STATE after a refit,
 * BDPT_E_INVALID for NULL.  In that mode _refit_check checks, in place of every triangle, every reference's eight mapped
 * region corners inside every decoded ancestor box. */
int bdpt_host_bvh_refit(void* handle, const float* positions);
int bdpt_host_bvh_refit_pieces(void* handle);
int bdpt_host_bvh_refit_check(void* handle, char* msg, uint32_t msgCap);
int bdpt_host_bvh_recs_hash(void* handle, uint64_t* out_hash);
int bdpt_host_bvh_refit_info(void* handle, bdpt_refit_info* out);
int bdpt_ctx_recs_hash(bdpt_ctx* ctx, uint64_t* out_hash);

/* Camera::calculateCameraParameters (Graphics/Camera/Camera.cpp:129-136) with
 * fovY = focalLengthToFovY (Utils/Math/FalcorMath.h:148-151).  Host-only helper. */
int bdpt_camera_look_at(const float pos[3], const float target[3], const float up[3], float focalLengthMm,
                        float frameHeightMm, float aspect, float focalDistance, bdpt_camera* out);

/* kMSAA jitter table shared by both passes (BDPTPass.cpp:20, LightProbeGBufferPass.cpp:36):
 * out = kMSAA[(frameCounterBeforeIncrement + 1) % 8] / 16 + 0.5. */
void bdpt_msaa_jitter(uint32_t frameCounterBeforeIncrement, float out[2]);

/* Size the per-pixel path state for a width×height frame of which rows
 * [tile.y0, tile.y1) are rendered here, at up to maxDepth. */
int bdpt_resize(bdpt_ctx* ctx, uint32_t width, uint32_t height, bdpt_tile tile, uint32_t maxDepth);

/* bdpt_resize for a tile made of interleaved stripes.  The splat buffer of such a context is OWNER-MAJOR: chunk o
 * (chunkU64 words, bdpt_tile_info) holds the accumulators of owner o's rows in row order, so a reduce-scatter over
 * the numOwners ranks leaves every rank with the summed accumulators of exactly its own pixels, in tile-local
 * order, ready for bdpt_resolve_tile.  (With bdpt_resize the buffer is in plain frame order.) */
int bdpt_resize_stripes(bdpt_ctx* ctx, uint32_t width, uint32_t height, bdpt_stripes stripes, uint32_t maxDepth);
/* The stripe height the tiled hosts of this build use for a frame of `height` rows dealt to `numOwners` ranks (C++
 * RenderingPipeline::setTiling, Python tiling.stripe_rows): small enough that every rank gets at least four stripes,
 * at most 8 rows — a stripe is only a run of rows in the tile's pixel list, so its size costs nothing, and small ones
 * spread the rows that cost most.  Host-only helper; any stripeRows >= 1 is valid for
 * bdpt_resize_stripes as long as all ranks agree. */
uint32_t bdpt_stripe_rows(uint32_t height, uint32_t numOwners);
int bdpt_get_tile_info(const bdpt_ctx* ctx, bdpt_tile_info* out);
/* The tile's rows as [first, last) pairs in ascending order; writes up to cap pairs, returns how many. */
int bdpt_tile_row_ranges(const bdpt_ctx* ctx, uint32_t* out_first_last, uint32_t cap);

/* Allocate optional per-frame buffers ahead of time, so that no execute call allocates (hipGraph capture,
 * first-frame latency): the built-in primary stage's channels and/or the BMFR history.  Call after
 * bdpt_resize (a resize frees them again).  Replaces the lazy texture creation of
 * ResourceManager::requestTextureResource / DenoisePass::initialize (SharedUtils/ResourceManager.cpp:210-241,
 * BidirectionalPathtracing/Passes/DenoisePass.cpp:60-96). */
#define BDPT_PREPARE_PRIMARY 1u
#define BDPT_PREPARE_BMFR 2u
#define BDPT_PREPARE_REFIT 4u /* the refit plan and scratch of bdpt_update_geometry now (needs a scene, not a size) */
#define BDPT_PREPARE_LIGHT_GROUPS 8u /* the per-light splat planes of bdpt_execute_light_groups (needs a scene and a size) */
#define BDPT_PREPARE_AREA_LIGHTS 16u /* the emitter table of BDPT_PARAM_AREA_LIGHTS (needs a scene, not a size) */
#define BDPT_PREPARE_LIGHT_GROUP_TABLE 32u /* numLights + 1 splat planes: the most an assignment of bdpt_execute_grouped needs */
#define BDPT_PREPARE_MOTION 64u /* the previous pose of bdpt_keep_pose, filled from the current one (needs a scene, not a size) */
#define BDPT_PREPARE_REFIT_PIECES 128u /* BDPT_PREPARE_REFIT plus the piece regions: later updates refit by pieces ("Animated scenes"; needs a scene, no update yet) */
int bdpt_prepare(bdpt_ctx* ctx, uint32_t what);

/* Primary-visibility pass.  Writes the tile rows of all six channels. */
int bdpt_gbuffer_execute(bdpt_ctx* ctx, const bdpt_gbuffer_params* p, const bdpt_gbuffer* out, void* stream);
/* The same plus the PrevWorldPosition channel ("Motion" above). */
int bdpt_gbuffer_execute_motion(bdpt_ctx* ctx, const bdpt_gbuffer_params* p, const bdpt_gbuffer* out, float* prevPosition, void* stream);

/* The BDPT pass.  `out` is the full-frame RGBA32F "PipelineOutput" channel;
 * only the tile rows are written (cleared to 0 first, as getClearedTexture does,
 * BDPTPass.cpp:73).  Without BDPT_PARAM_DEFER_RESOLVE the splats of this call are
 * folded in before returning control to the stream.
 * `in` may be NULL: the primary stage then runs inside the call into channels the context owns
 * (pinhole, p->pixelJitter, p->frameCount, default constant environment).  They are allocated by
 * bdpt_prepare(BDPT_PREPARE_PRIMARY), or else by the first such call — which therefore must not be
 * inside a stream capture (BDPT_E_STATE). */
int bdpt_execute(bdpt_ctx* ctx, const bdpt_params* p, const bdpt_gbuffer* in, float* out, void* stream);

/* Light groups (light AOVs): bdpt_execute plus the frame broken down by light source, from the same paths and the same
 * rays.  `groups` is device memory of (numLights + 1) x W x H RGBA32F planes, each laid out like `out`: plane k < numLights
 * is light k (the scene's order), plane numLights is emission.  Every term of the frame has exactly one source — a
 * next-event term the light drawn for it, a light-tracing splat and every connection the light the pixel's light subpath
 * starts at, the G-buffer emissive, the background and the ENV_ON_MISS / EMISSIVE_HITS terms none — and paths, random
 * draws, rays and w never depend on intensities.  Hence, bit for bit:
 *   - `out` is what bdpt_execute writes, and the ray counters are the same;
 *   - the emission plane (all four channels) is the bdpt_execute frame with every light's intensity zero;
 *   - light plane k's RGB is the bdpt_execute frame with every other light's intensity zero, the G-buffer emissive RGB
 *     zero, the background pixels' diffuse RGB zero and ENV_ON_MISS / EMISSIVE_HITS cleared;
 *   - every plane's w is out.w.
 * The planes add up to `out` only up to float reassociation, and only where `out` never saturates: each plane saturates
 * on its own sums (the connection writes and the splat fold-in clamp to [0, 1]), as the frame it equals does.
 * Ordering, stream use and in == NULL are those of bdpt_execute.  The per-light splat planes (numLights x W x H x 32 B,
 * cleared every frame) are allocated by bdpt_prepare(BDPT_PREPARE_LIGHT_GROUPS) or by the first call, which then must not
 * be inside a stream capture (BDPT_E_STATE); after the prepare the call allocates nothing and can be captured.
 * bdpt_set_scene and bdpt_resize free them.
 * Errors: a NULL ctx or groups BDPT_E_INVALID; BDPT_PARAM_DEFER_RESOLVE or BDPT_PARAM_DEFER_TAIL BDPT_E_INVALID; no scene
 * or size BDPT_E_STATE; a context that renders a tile or stripes (not the whole frame) BDPT_E_INVALID — the splat
 * exchange of tiled rendering has no group planes. */
int bdpt_execute_light_groups(bdpt_ctx* ctx, const bdpt_params* p, const bdpt_gbuffer* in, float* out, float* groups, void* stream);

/* Assignable light groups: the breakdown above with a caller's table from light to group ("key", "fill", "practicals"),
 * and with the emitter table of BDPT_PARAM_AREA_LIGHTS as one more light, "light numLights".  The cost follows the number
 * of groups, not of lights: numGroups + 1 planes are written and numGroups splat-value planes cleared.
 * `planes` is device memory of (numGroups + 1) x W x H RGBA32F planes: plane g < numGroups is group g, plane numGroups is
 * emission.  `groupOf` is a HOST array of numAssigned bytes, copied before the call returns (a captured graph holds the
 * copy): groupOf[i] is the group of light i, and with BDPT_PARAM_AREA_LIGHTS groupOf[numLights] that of the emitter table.
 * Sources of terms: a next-event term belongs to the light drawn for it; a splat and every connection to the light the
 * pixel's light subpath starts at; either light may be the table.  The G-buffer emissive, the background and the
 * ENV_ON_MISS / EMISSIVE_HITS terms have no source and go to the emission plane.  Paths, random draws, rays and w never
 * depend on intensities or on emission.  Hence, bit for bit:
 *   - `out` and the ray counters are bdpt_execute's for the same params, BDPT_PARAM_AREA_LIGHTS included;
 *   - every plane's w is out.w;
 *   - group plane g's RGB is the bdpt_execute frame in which every source outside g contributes exactly +0 — every draw,
 *     path and ray stays the same — with the G-buffer emissive RGB and the background pixels' diffuse RGB zero and
 *     ENV_ON_MISS / EMISSIVE_HITS cleared; several lights of one group sum their terms in that frame's order;
 *   - a group may be empty: its plane is (0, 0, 0, w);
 *   - the emission plane is the frame in which every source contributes +0;
 *   - the identity assignment (numGroups = numLights, groupOf[i] = i) without the switch gives
 *     bdpt_execute_light_groups' planes, `out` and counters.
 * The area-light switch: without it numAssigned is numLights; with it numAssigned is numLights + 1, and the last entry is
 * read only while the table's W > 0 — with no emitter or W == 0 the switch changes nothing, as everywhere else (the
 * entry must still name a group).  The emitter table is made as bdpt_execute makes it (bdpt_prepare(
 * BDPT_PREPARE_AREA_LIGHTS) or the first frame with the switch).
 * Ordering, stream use, in == NULL and capture are those of bdpt_execute_light_groups.  The call needs numGroups
 * splat-value planes (W x H x 32 B each): bdpt_prepare(BDPT_PREPARE_LIGHT_GROUPS) allocates numLights of them,
 * bdpt_prepare(BDPT_PREPARE_LIGHT_GROUP_TABLE) numLights + 1, the most any assignment needs; a call that finds too few
 * allocates them (it waits for the device first) and then must not be inside a stream capture (BDPT_E_STATE, nothing
 * enqueued).
 * Errors (nothing is enqueued): a NULL ctx, params, out, desc, planes or groupOf BDPT_E_INVALID; numGroups 0 or above
 * BDPT_MAX_LIGHTS + 1, numAssigned not as stated, an entry >= numGroups, non-zero reserved BDPT_E_INVALID;
 * BDPT_PARAM_DEFER_RESOLVE / _DEFER_TAIL BDPT_E_INVALID; BDPT_PARAM_AREA_LIGHTS with BDPT_PARAM_MIS_POWER / _LINEAR
 * BDPT_E_INVALID; a context that renders a tile or stripes BDPT_E_INVALID; no scene or size BDPT_E_STATE.
 * bdpt_execute_light_groups itself keeps refusing BDPT_PARAM_AREA_LIGHTS (its buffer has no plane for the table). */
typedef struct bdpt_light_group_desc {
  float* planes;          /* device: (numGroups + 1) x W x H RGBA32F; plane g < numGroups = group g, plane numGroups = emission */
  uint32_t numGroups;     /* 1 .. BDPT_MAX_LIGHTS + 1 */
  uint32_t numAssigned;   /* entries of groupOf: numLights, or numLights + 1 when p->flags has BDPT_PARAM_AREA_LIGHTS */
  const uint8_t* groupOf; /* HOST array, copied before the call returns: the group of light i; entry numLights = the emitter table */
  uint32_t reserved[2];   /* 0 */
} bdpt_light_group_desc;
int bdpt_execute_grouped(bdpt_ctx* ctx, const bdpt_params* p, const bdpt_gbuffer* in, float* out, const bdpt_light_group_desc* desc,
                         void* stream);

/* Masked frame (region of interest, foveation, adaptive sampling): bdpt_execute for the pixels `mask` selects.  `mask` is
 * device memory of W x H bytes in frame order; a non-zero byte makes the pixel ACTIVE.  Bit for bit:
 *   - an active pixel (any G-buffer state) gets exactly what bdpt_execute writes for the same params, G-buffer and scene;
 *   - an inactive pixel's `out` is not written: its previous bits survive.
 * Why this holds: every term of pixel p depends only on p's own eye and light subpaths, seeded by initRand(pix,
 * frameCount) and, for NEE, by seedL; the one exception, light-tracing splats, land on other pixels.  So every valid
 * pixel still traces its LIGHT subpath and its splats land, and an inactive pixel drops its eye walk, its NEE, connection
 * and lazy-round rays, its gather and its `out` writes (the emissive / background write included, and the resolve).
 * MIS: with BDPT_PARAM_MIS_POWER or _LINEAR the splat weight of p's light subpath reads p's EYE prefix products, so then
 * inactive valid pixels still walk their eye subpaths (and run the MIS prefix pass) and skip only NEE, connections,
 * gather and lazy rounds; with ENV_ON_MISS / EMISSIVE_HITS also on, their eye walk adds nothing to `out`.
 * Counters: raysLightExtend, raysSplat, splatsLanded and hintedSplat are bdpt_execute's; raysEyeExtend (MIS off),
 * raysNee, raysConnect, raysConnectLazy and hintedNee count active pixels only, pixelsValid active valid pixels.  With
 * MIS off and an all-zero mask the first four are 0; with MIS on raysEyeExtend is bdpt_execute's.
 * Ordering, stream use, in == NULL and graph capture are those of bdpt_execute; the call allocates nothing beyond what
 * bdpt_execute does (in == NULL: bdpt_prepare(BDPT_PREPARE_PRIMARY) before a capture).
 * Errors: a NULL ctx or mask BDPT_E_INVALID; BDPT_PARAM_DEFER_RESOLVE or BDPT_PARAM_DEFER_TAIL BDPT_E_INVALID; no scene
 * or size BDPT_E_STATE; a context that renders a tile or stripes BDPT_E_INVALID (the eye list is whole-frame). */
int bdpt_execute_masked(bdpt_ctx* ctx, const bdpt_params* p, const bdpt_gbuffer* in, const uint8_t* mask, float* out, void* stream);

/* Adaptive sampling: a per-pixel running mean and variance, and the mask of the next masked frame.  All buffers are
 * caller-owned device memory over the whole frame, in frame order. */
typedef struct bdpt_adaptive_state {
  float* mean;      /* RGBA32F running mean (what bdpt_accumulate's lastFrame holds); 16-byte aligned */
  float* m2;        /* float32 per pixel: summed squared luminance deviations */
  uint32_t* count;  /* frames folded into each pixel */
  uint8_t* mask;    /* 1 = render next frame: the mask bdpt_execute_masked reads */
  uint32_t* active; /* one word: pixels with mask 1 after the last reset / update */
} bdpt_adaptive_state;
typedef struct bdpt_adaptive_params {
  float threshold;     /* relative standard error of the mean at which a pixel has converged */
  float epsilon;       /* added to the mean luminance in the denominator */
  uint32_t minSamples; /* >= 2 */
  uint32_t maxSamples; /* >= minSamples; a pixel at maxSamples has converged */
  uint32_t blockSize;  /* 1, 2, 4, 8 or 16: pixels are (de)activated per aligned blockSize x blockSize block */
} bdpt_adaptive_params;
/* mean = m2 = count = 0, mask = 1 everywhere, *active = W * H. */
int bdpt_adaptive_reset(bdpt_ctx* ctx, const bdpt_adaptive_state* s, void* stream);
/* Folds `frame` (RGBA32F, the masked frame's `out`) into the state, decides the next mask and writes the mean back to
 * `frame`.  fp32 throughout, in exactly this order (no contraction, correctly rounded / and sqrtf):
 *   lum(v) = (0.2126f*v.x + 0.7152f*v.y) + 0.0722f*v.z
 *   for every pixel with mask != 0 and count < maxSamples, with n = count, c = frame, a = (float)n, b = (float)(n+1):
 *     mean' = (a*mean + c)/b                      per channel, all four (bdpt_accumulate's expression: a pixel that is
 *                                                 always active follows bdpt_accumulate bit for bit)
 *     m2    = m2 + (lum(c) - lum(mean)) * (lum(c) - lum(mean'))     (mean the old mean)
 *     mean  = mean';  count = n + 1
 *   converged = count >= maxSamples, or count >= minSamples and
 *               sqrtf(m2 / (nf*(nf - 1.0f))) / (lum(mean) + epsilon) <= threshold,  nf = (float)count
 *               (for every pixel, rendered this frame or not; a NaN comparison is "not converged")
 *   mask   = 1 for every pixel of an aligned blockSize^2 block that holds any unconverged pixel, else 0 (partial blocks at
 *            the right and bottom edges count their real pixels only)
 *   active = the number of pixels with mask 1
 *   frame  = mean for every pixel, so that the output always shows the accumulated image; an inactive pixel, which the
 *            next masked frame leaves untouched, keeps showing its mean.
 * The edges, all of them the lines above taken literally:
 *   - mask: any non-zero byte is "render"; the update itself writes 0 and 1 only.
 *   - counts: the test count < maxSamples and the increment are exact in 32 bits (maxSamples up to 2^32 - 1); only the
 *     casts a, b and nf round, to nearest even from 2^24 + 1 on.  A pixel whose count is already beyond maxSamples is left
 *     alone and is converged.
 *   - the comparison is made as written, whatever its sides are.  A quotient that is negative because
 *     lum(mean) + epsilon < 0 is <= a threshold >= 0: converged.  lum(mean) + epsilon == 0 gives +inf (not converged
 *     unless the threshold is +inf) or, with m2 == 0, NaN.  m2 < 0 (rounding of a pixel whose frames agree to an ulp, or a
 *     caller's state) makes sqrtf NaN: not converged before maxSamples.  A NaN threshold never converges before
 *     maxSamples; nor does a negative one, but for a negative quotient below it; a threshold of 0 or -0.0 converges
 *     exactly where the quotient is 0 or negative; +inf converges every quotient but NaN at minSamples.
 *   - non-finite frames, means and m2 propagate by IEEE rules; which NaN a NaN is, is not promised.
 * A block that turns inactive never turns active again (its pixels no longer change), so `active` never grows between
 * resets.  The call neither allocates nor synchronises (read `active` by an async copy) and can be captured; it is ordered
 * behind the context's previous call.  Errors: a NULL ctx, params, state buffer or frame, a blockSize not in
 * {1, 2, 4, 8, 16}, minSamples < 2 or maxSamples < minSamples BDPT_E_INVALID; no scene or size BDPT_E_STATE; a tile or
 * stripes context BDPT_E_INVALID. */
int bdpt_adaptive_update(bdpt_ctx* ctx, const bdpt_adaptive_params* a, const bdpt_adaptive_state* s, float* frame, void* stream);

/* Second phase of a bdpt_execute issued with BDPT_PARAM_DEFER_TAIL (same params, channels and out). */
int bdpt_execute_tail(bdpt_ctx* ctx, const bdpt_params* p, const bdpt_gbuffer* in, float* out, void* stream);

/* Full-frame fixed-point splat accumulator: uint64[4] per pixel (r,g,b in
 * 2^-32 units, splat count) in frame order (bdpt_resize) or owner-major order (bdpt_resize_stripes),
 * zeroed by every bdpt_execute before its splat stage.
 * Exposed so a multi-GPU host can sum it across ranks (integer sum: exact and
 * order-independent) before bdpt_resolve. */
int bdpt_splat_buffer(bdpt_ctx* ctx, uint64_t** out_device_ptr, uint64_t* out_num_u64);

/* Make the pass accumulate splats into caller-owned device memory (e.g. a tensor that a
 * collective library can reduce in place); NULL restores the context's own buffer. */
int bdpt_set_splat_buffer(bdpt_ctx* ctx, uint64_t* device_ptr, uint64_t num_u64);

/* out[tile rows] = saturate(out + splat) where the splat count is non-zero.
 * `splat` may be the context's own buffer or a reduced copy holding at least the
 * tile rows at the same full-frame indexing (splat_row0 = first row it holds).
 * fp32, per channel, in exactly this order:
 *   v     = (float)word * 2^-32f    the conversion of the 64-bit word rounds ONCE, to nearest even (never through a
 *                                   double: 2^63 + 2^39 + 1 becomes 2^63 + 2^40); the scaling is exact
 *   out.c = saturate(out.c + v)     saturate(x) = min(max(x, 0), 1) with saturate(NaN) = +0 and saturate(-0) = +0
 *   out.w = saturate(out.w + (float)count)
 * Whatever `out` holds is used as it is (negative, beyond 1, infinite, NaN): the result is in [0, 1] and never a NaN.
 * A pixel whose count word is 0 is neither read nor written, whatever its colour words hold. */
int bdpt_resolve(bdpt_ctx* ctx, const uint64_t* splat, uint32_t splat_row0, float* out, void* stream);

/* The same for a buffer that holds the tile's accumulators in tile-local order (4 uint64 per tile pixel): one
 * owner's chunk after the reduce-scatter of an owner-major splat buffer. */
int bdpt_resolve_tile(bdpt_ctx* ctx, const uint64_t* tile_splat, float* out, void* stream);

/* Running mean of accumulate.ps.hlsl:28-42 over `numTexels` RGBA32F texels:
 *   cur = accumCount < maxAccumCount ? (accumCount*last + cur)/(accumCount+1) : last;  last = cur.
 * fp32 in that order (product, sum, correctly rounded quotient; no contraction; subnormals kept), with
 * a = (float)accumCount and b = (float)(accumCount + 1), casts that round to nearest even from 2^24 + 1 on.  IEEE
 * throughout: 0 * inf is NaN (count 0 does not hide a non-finite `last`), a * last may overflow to an infinity where the
 * mean itself is finite, and which NaN a NaN result is, is not promised. */
int bdpt_accumulate(bdpt_ctx* ctx, float* lastFrame, float* curFrame, uint32_t accumCount, uint32_t maxAccumCount,
                    uint64_t numTexels, void* stream);

/* The same running mean restricted to this context's tile: lastFrame / curFrame are full-frame RGBA32F buffers, only
 * the tile's pixels are read and written (one launch, whatever the number of stripes). */
int bdpt_accumulate_tile(bdpt_ctx* ctx, float* lastFrame, float* curFrame, uint32_t accumCount, uint32_t maxAccumCount, void* stream);

/* ---- BMFR denoiser (DenoisePass.*).  Works on the full frame: the context's tile must cover it. ---- */
#define BDPT_BMFR_PREPROCESS 1u        /* mBMFR_preprocess, default on (DenoisePass.h:72) */
#define BDPT_BMFR_REGRESSION 2u        /* mBMFR_regression, default off (DenoisePass.h:74) */
#define BDPT_BMFR_POSTPROCESS 4u       /* mBMFR_postprocess, default on (DenoisePass.h:73) */
#define BDPT_BMFR_KEEP_LD_FEATURES 8u  /* mBMFR_removeFeatures == false: plain Householder QR with feature noise */
#define BDPT_BMFR_FULL_FRAME 16u       /* deviation switch: the reference filters only texC.x <= 0.5 (its comparison split) */

typedef struct bdpt_bmfr_params {
  uint32_t frameNumber;   /* mAccumCount: 0 on the first frame after bdpt_bmfr_reset */
  uint32_t flags;         /* BDPT_BMFR_* */
  float prevViewProj[16]; /* gCamera.prevViewProjMat, row-major: clip[r] = sum_c m[4r+c] * (posW,1)[c] */
} bdpt_bmfr_params;

/* One execute() of the denoise pass on `noisy` (full-frame RGBA32F, in/out: the channel being
 * denoised) with the G-buffer's WorldPosition / WorldNormal / MaterialDiffuse as features.  History
 * (previous position, normal, noisy and filtered frames, accept masks) lives in the context; it is allocated
 * by bdpt_prepare(BDPT_PREPARE_BMFR) or by the first call (not inside a stream capture: BDPT_E_STATE).
 * The filter's blocks need their neighbours, so ALL FOUR buffers must hold the WHOLE frame, also when the context
 * renders only a band or the stripes of one rank: a tiled host gathers them first (bdpt_tile_pack -> all-gather ->
 * bdpt_tile_unpack; host/Passes.cpp BlockwiseMultiOrderFeatureRegression::execute) and every rank filters the same
 * whole frame.
 * Non-finite and background texels follow the shaders under D3D rules: max / min return the operand that is not a NaN,
 * int() of a float rounds toward zero, gives 0 for a NaN and saturates, a load outside a texture is 0.  So a texel whose
 * reprojection is 0/0 (a worldPosition of (0,0,0) seen from a previous camera at the origin) passes the "outside" test and
 * tests the four taps around pixel (0,0) with NaN weights; a NaN position or normal fails every tap test and leaves that
 * texel's colour as it came; in the regression a NaN feature does not decide its block's range, the default QR drops the
 * column that holds it and leaves the NaN to its own texel, while an infinite feature, any non-finite feature under
 * BDPT_BMFR_KEEP_LD_FEATURES, or a non-finite colour (its own channel) makes the whole block NaN.  Where an input makes a
 * result a NaN, a NaN is promised, not which one. */
int bdpt_bmfr_execute(bdpt_ctx* ctx, const bdpt_bmfr_params* p, const bdpt_gbuffer* features, float* noisy, void* stream);

/* bdpt_bmfr_execute for scenes whose geometry moves.  prevPosition (device, 16-byte aligned, whole-frame float4 texels:
 * bdpt_gbuffer_execute_motion's channel; NULL: BDPT_E_INVALID) says where each pixel's surface point was in the previous
 * frame.  With q = prevPosition[i] and cp = features->worldPosition[i], the preprocess stage projects q (not cp) with
 * prevViewProj and accepts a history tap when |tap position - q|^2 < 0.01 (not cp).  Everything else is
 * bdpt_bmfr_execute's: the normal test against the current normal, the weights, the blend, the accept masks, the history
 * write (which stores the CURRENT position cp), regression and postprocess (which read `features`), history allocation,
 * whole-frame buffers, the history blob.  With prevPosition equal to worldPosition the call is bdpt_bmfr_execute bit for
 * bit.  Rotating surfaces still fail the normal test: normals are not reprojected. */
int bdpt_bmfr_execute_motion(bdpt_ctx* ctx, const bdpt_bmfr_params* p, const bdpt_gbuffer* features, const float* prevPosition,
                             float* noisy, void* stream);

/* Forget the history (BlockwiseMultiOrderFeatureRegression::resize / initScene set mAccumCount = 0). */
int bdpt_bmfr_reset(bdpt_ctx* ctx);

/* The denoiser's state that crosses frames — the previous frame's position, normal, noisy and filtered images, what the
 * next bdpt_bmfr_execute reads — as one host blob, so that a host can checkpoint a pipeline with the denoiser on
 * (the reference keeps these in textures of the pass, DenoisePass.h:40-66, and has no checkpoints at all).
 * bdpt_bmfr_history_bytes: the blob's size for this context's frame (0 before the history exists).
 * save: synchronises the last stream used; `bytes` must be at least that size.  load: allocates the history if need
 * be; `bytes` must be exactly that size (BDPT_E_INVALID otherwise: a blob of another frame size). */
int bdpt_bmfr_history_bytes(const bdpt_ctx* ctx, uint64_t* out_bytes);
int bdpt_bmfr_save_history(bdpt_ctx* ctx, void* host_blob, uint64_t bytes);
int bdpt_bmfr_load_history(bdpt_ctx* ctx, const void* host_blob, uint64_t bytes);

/* ---- Denoised planes: several images over one G-buffer (light-group planes, for relighting) with one fit ----
 * bdpt_bmfr_execute_planes denoises numPlanes whole-frame images that share `features` in one call: the reprojection
 * and its geometry tests, the feature scaling and the Householder factorisation of the ten feature columns of every
 * block are done once, the colour work per plane.  bdpt_bmfr_execute and bdpt_bmfr_execute_motion are the one-plane case
 * of the same code, on a history of their own.
 *
 * Contract.  After the call planes[k] holds exactly the bits bdpt_bmfr_execute (with prevPosition set:
 * bdpt_bmfr_execute_motion) would have left in it on a context of its own that was fed planes[k], the same `features`
 * and the same params on every frame since its reset — for every flag combination bdpt_bmfr_execute accepts (regression
 * off, BDPT_BMFR_KEEP_LD_FEATURES, BDPT_BMFR_FULL_FRAME, stages switched off).  List position k owns history slot k.
 * Colours, w / spp, sampleSpp and both blend factors are computed per plane from that plane's own history; only what
 * reads positions and normals alone is shared.
 *
 * History.  The plane history is apart from the single-image history and laid out like it, which is the one-slot case:
 * position and normal ping-pong pairs, the accept mask and prevPixel once, noisy and filtered ping-pong pairs per slot.
 * bdpt_bmfr_execute, _motion, _reset, _history_bytes, _save_history and _load_history keep their bits and their state
 * whatever is called here, and the blob functions cover the single-image history only: the plane history is not
 * checkpointed.  bdpt_resize drops it, as it drops the other.
 *   bdpt_bmfr_planes_prepare(n)  allocates the history for n planes (if fewer are there) and resets it.
 *   bdpt_bmfr_planes_reset       forgets it (BDPT_OK when there is none).
 * A call that needs more planes than are allocated waits for the device, reallocates and resets the plane history
 * (inside a stream capture: BDPT_E_STATE, as the other first-use allocations); one with fewer uses the first numPlanes
 * slots.  Stream capture follows bdpt_bmfr_execute's rule: history prepared beforehand, the ping-pong side chosen on the
 * host at capture time.
 *
 * Errors, nothing enqueued on any: no size BDPT_E_STATE; a NULL ctx, params, features or desc, missing feature channels,
 * numPlanes outside 1 .. BDPT_BMFR_MAX_PLANES, non-zero reserved, a NULL or misaligned plane or a misaligned
 * prevPosition, two planes whose byte ranges overlap BDPT_E_INVALID.  As bdpt_bmfr_execute, the call takes WHOLE-FRAME
 * buffers also on a band or stripes context. */
#define BDPT_BMFR_MAX_PLANES (BDPT_MAX_LIGHTS + 2) /* 16 groups + emission + the frame itself */
typedef struct bdpt_bmfr_planes_desc {
  float* const* planes;      /* HOST array of numPlanes device pointers; each a whole-frame RGBA32F image, 16-byte aligned,
                                in/out; the array is copied before the call returns (as groupOf is) */
  uint32_t numPlanes;        /* 1 .. BDPT_BMFR_MAX_PLANES */
  uint32_t reserved;         /* 0 */
  const float* prevPosition; /* optional: bdpt_bmfr_execute_motion's channel; NULL = bdpt_bmfr_execute's reprojection */
} bdpt_bmfr_planes_desc;
int bdpt_bmfr_execute_planes(bdpt_ctx* ctx, const bdpt_bmfr_params* p, const bdpt_gbuffer* features,
                             const bdpt_bmfr_planes_desc* desc, void* stream);
int bdpt_bmfr_planes_prepare(bdpt_ctx* ctx, uint32_t numPlanes); /* allocate + reset the plane history */
int bdpt_bmfr_planes_reset(bdpt_ctx* ctx);

/* Rows of a tile as one contiguous run, and back: `frame` is a whole-frame buffer of `bytesPerPixel` (4, 8 or 16) bytes
 * per pixel, `packed` holds rows of `width` pixels.
 * bdpt_tile_pack:   packed[i] = frame[pixel i of this context's tile] (its rows in ascending order: the order of a
 *                   stripes context's chunk of an all-gather).
 * bdpt_tile_unpack: the rows of owner `owner` of this context's stripe layout (bdpt_resize_stripes; a band context has
 *                   the one owner 0) go from `packed` (numRows of that owner, in order; rows the padding of a chunk
 *                   stands for lie outside the frame and are skipped) back to their places in `frame`.
 * What a tiled host needs around an all-gather of tile framebuffers when the gathered frame
 * stays on the device (the denoiser); RenderingPipeline::readOutput does the same on the host. */
int bdpt_tile_pack(bdpt_ctx* ctx, const void* frame, void* packed, uint32_t bytesPerPixel, void* stream);
int bdpt_tile_unpack(bdpt_ctx* ctx, uint32_t owner, const void* packed, void* frame, uint32_t bytesPerPixel, void* stream);

/* projMat * viewMat of Falcor's camera without the jitter matrix (glm::perspective * glm::lookAt,
 * Camera.cpp:77-105), row-major as bdpt_bmfr_params::prevViewProj wants it.  Host only. */
int bdpt_camera_view_proj(const float pos[3], const float target[3], const float up[3], float focalLengthMm,
                          float frameHeightMm, float aspect, float nearZ, float farZ, float out16[16]);

/* Counters of the most recent bdpt_execute (ray tallies always; node/triangle visits when it ran
 * with BDPT_PARAM_COUNTERS).  Synchronises the stream it was launched on. */
int bdpt_get_counters(bdpt_ctx* ctx, bdpt_counters* out);

/* Per-stage device time (ms) of the most recent bdpt_execute, measured with
 * HIP events on the launch stream.  names/ms hold up to `cap` entries; returns
 * the number written (>= 0) or a negative error.  A stage of the launch stream is one kernel ("walk", "gen_nee",
 * "trace_terms", "trace_pairs", "gather", "lazy_gen", "lazy_trace" ...), one group of memsets ("clear") or a wait for
 * the context's second stream ("splat_wait", "connect_wait"); their sum is the frame's critical path.  The kernels of
 * the second stream follow with names that start with "side:" ("side:gen_splat", "side:gen_connect"), timed by event
 * pairs on that stream: they run beside the stages above and are not part of that sum. */
int bdpt_get_stage_times(bdpt_ctx* ctx, const char** names, float* ms, int cap);
int bdpt_enable_stage_timing(bdpt_ctx* ctx, int enable);

int bdpt_sync(bdpt_ctx* ctx, void* stream);

/* The emitter table of BDPT_PARAM_AREA_LIGHTS (made here if need be; synchronises): emitters, of which textured, and W as
 * of the last bdpt_update_geometry.  No scene BDPT_E_STATE. */
typedef struct bdpt_area_light_info {
  uint32_t numEmitters;
  uint32_t numTextured;
  float totalWeight; /* W */
  uint32_t reserved;
} bdpt_area_light_info;
int bdpt_get_area_light_info(bdpt_ctx* ctx, bdpt_area_light_info* out);

/* Test hooks through the same library (used by the parity tests; they launch
 * the device functions of the hot path on caller-supplied inputs). */
/* initRand/nextRand stream: out[i*draws + k] = k-th nextRand seed state for (val0[i], val1[i]). */
int bdpt_test_rng(bdpt_ctx* ctx, const uint32_t* val0, const uint32_t* val1, uint32_t n, uint32_t draws,
                  uint32_t* out_states, float* out_floats);
/* Closest-hit / any-hit queries on host ray arrays (origin xyz, dir xyz, tmin, tmax per ray).
 * hit: prim (int32, -1 miss), t, u, v per ray.  mode 0 closest, 1 closest+cull-back, 2 any-hit (prim = 0/-1). */
int bdpt_test_trace(bdpt_ctx* ctx, const float* rays, uint32_t n, int mode, int32_t* out_prim, float* out_tuv);
/* The persistent any-hit kernel (the one the pass uses for NEE, splat and connection rays) over host rays of the same
 * layout; tmin is taken from ray 0.  out_vis: 1 = unoccluded.  out_max_stack (may be NULL): deepest traversal stack any
 * ray reached — entries beyond the LDS rows live in the context's overflow area (kernels.h kStackLds). */
int bdpt_test_trace_shadow(bdpt_ctx* ctx, const float* rays, uint32_t n, uint8_t* out_vis, uint32_t* out_max_stack);
/* BSDF known-answer hook: inputs are n records of 20 floats
 * (N3 V3 L3 dif3 spec3 rough isSpecular seed(bits) pad2); outputs n records of 16 floats
 * (sampleBRDF: weight3 L3 pdf isSpec | evalBRDF: f3 | pad).  matIndex bit 1 = BDPT_PARAM_SPECULAR_FROM_LOBE. */
int bdpt_test_bsdf(bdpt_ctx* ctx, const float* in, uint32_t n, uint32_t matIndex, float* out);
/* Area-light known-answer hook: the device functions the AREA instances of init_paths and gen_nee run, on host arrays;
 * synchronous.  states[i]: the RNG state right after the selection draw.  out: 16 floats per item (integers as bits).
 *   mode 0 (light subpath start): prim, b1, b2, pos.xyz, side normal n.xyz, direction.xyz, colour.xyz, seedL (the state
 *          after the draws)
 *   mode 1 (NEE sample; points[i]: the receiving point, 3 floats): prim, L.xyz, d, intensity.xyz, b1, b2, x.xyz, 0, 0, 0
 * With no emitter or W == 0 every output is 0.  Errors: mode > 1, a NULL array BDPT_E_INVALID; no scene BDPT_E_STATE. */
int bdpt_test_area_light_sample(bdpt_ctx* ctx, uint32_t mode, const uint32_t* states, const float* points, uint32_t n, float* out);
/* Alpha-test known-answer hook: the any-hit alpha verdict of candidate (prim[i], uv[2i], uv[2i+1]) from the device functions
 * the traversal calls, one lane per item, on host arrays; synchronous.  out_fails[i] = 1 where the candidate is ignored; an
 * opaque triangle passes.  variant 0: alphaTestFails; 1: alphaTestFails2 with the item in the first slot and item i + 1
 * (item 0 after the last) in the second; 2: the item in the second slot, the partner in the first with its test switched
 * off.  Errors: a NULL array, variant > 2 or a prim >= numTriangles BDPT_E_INVALID; no scene BDPT_E_STATE. */
int bdpt_test_alpha(bdpt_ctx* ctx, uint32_t variant, const uint32_t* prim, const float* uv, uint32_t n, uint8_t* out_fails);
/* Skinning measurement hook: the skinning kernel of bdpt_update_skinned alone, enqueued on `stream` behind the context's
 * previous call, with the context's device palette as the last BDPT_MEMORY_HOST update staged it (no refit: the scene is
 * left as it was, the skinned streams are rewritten).  path 0: the path bdpt_update_skinned takes, 1: the global-memory
 * gather, 2: the LDS-staged palette (where the palette is small enough for it, else the gather).  Errors: no skin
 * BDPT_E_STATE, path > 2 BDPT_E_INVALID. */
int bdpt_test_skin_kernel(bdpt_ctx* ctx, uint32_t path, void* stream);
/* Morph measurement hook: the morph kernel of bdpt_update_morphed alone, enqueued on `stream` behind the context's
 * previous call, with the context's device weights and palettes as the last BDPT_MEMORY_HOST update staged them (no
 * refit: the scene is left as it was, the output streams are rewritten).  path as bdpt_test_skin_kernel's: 0 the path
 * bdpt_update_morphed takes, 1 the global-memory palette gather, 2 the LDS-staged palette (with a skin whose palette is
 * small enough for it, else the gather).  Errors: no morph BDPT_E_STATE, path > 2 BDPT_E_INVALID. */
int bdpt_test_morph_kernel(bdpt_ctx* ctx, uint32_t path, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BDPT_H_ */
