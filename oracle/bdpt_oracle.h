/*
 * bdpt_oracle.h — CPU ORACLE.  TEST INFRASTRUCTURE, NOT PRODUCT.
 *
 * Scalar C++17 restatement of the reference's bidirectional path-tracing pass
 * (SunBangjie/FYP-BidirectionalPathTracer).  Only tests/, __graft_entry__.smoke()
 * and bench.py's cpu_baseline leg may load this library; nothing under
 * fyp-bidirectionalpathtracer_amd/ links, imports or calls it.
 *
 * Parity pinning status: the reference holds no golden vectors,
 * known-answer tests or rendered images for this path and cannot be built or run
 * here (HLSL/DXR + D3D12, Windows-only; toolchain and dependencies absent), so
 *   - the integrator arithmetic (RNG, BSDF sampling/eval, NEE, splat, connection,
 *     accumulation) is a line-by-line restatement of the cited shader lines and is
 *     self-pinned by the fixtures under tests/golden/ that this oracle generated
 *     (tests/golden/make_golden.py);
 *   - BVH traversal, ray/triangle intersection, texture filtering and the
 *     float->half G-buffer rounding live in the DXR driver / sampler hardware with
 *     no source in the reference: for those, PARITY IS UNPINNED and the oracle's
 *     definition (Moeller-Trumbore, brute-force cross-check, bilinear/wrap,
 *     round-to-nearest-even) is the build's own.
 *
 * Scene / camera / parameter structs are the product ABI's (include/bdpt.h) so
 * both sides consume byte-identical inputs.
 */
#ifndef BDPT_ORACLE_H_
#define BDPT_ORACLE_H_

#include <stdint.h>

#include "../include/bdpt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct oracle_scene oracle_scene;

/* Copies the scene, builds the oracle's own (median-split) BVH. */
oracle_scene* oracle_scene_create(const bdpt_scene_desc* desc);
void oracle_scene_destroy(oracle_scene* s);
/* Environment for BDPT_PARAM_ENV_ON_MISS (include/bdpt.h); envMap is a HOST pointer here and is copied. NULL = black. */
void oracle_set_environment(oracle_scene* s, const bdpt_environment* env);

#define ORACLE_BRUTE_FORCE 1u /* intersect every triangle instead of using the BVH */
/* Cross-check hook (tests/test_oracle_cross_check.py): treat every vertex-connection shadow ray as unoccluded.
 * The reference ends those rays exactly ON the far surface (tmax = |B-A|, BDPTMain.rt.hlsl:222-223), so whether
 * the far surface itself occludes them is decided by the last bit of the arithmetic; with this flag the
 * connection sums can be compared with an implementation in another precision. */
#define ORACLE_CONNECT_ALL_VISIBLE 2u
/* The same hook for the next-event and light-tracing shadow rays (tests/test_edge_scenes_cpu.py): a light that lies ON a
 * surface, or a camera on one, ends every such ray on that surface, the same last-bit decision. */
#define ORACLE_TERMS_ALL_VISIBLE 4u

typedef struct oracle_frame {
  uint32_t width, height;
  uint32_t y0, y1; /* rows rendered */
  /* Full-frame host buffers (width*height texels).  G-buffer channels hold the
   * values the BDPT pass would read back: position fp32, others fp16-rounded. */
  float* worldPosition;     /* 4 floats/texel */
  float* worldNormal;       /* 4 */
  float* materialDiffuse;   /* 4 */
  float* materialSpecRough; /* 4 */
  float* materialExtra;     /* 4 */
  float* emissive;          /* 4 */
  float* out;               /* 4: own-pixel terms, then resolved */
  uint64_t* splat;          /* 4 u64/texel, full frame; caller zeroes */
} oracle_frame;

/* G-buffer pass for rows [y0,y1). */
int oracle_gbuffer(const oracle_scene* s, const bdpt_camera* cam, const bdpt_gbuffer_params* gp,
                   const float* envMapHost, oracle_frame* f, uint32_t flags, int threads);

/* BDPT pass for rows [y0,y1): own-pixel terms into f->out, splats into f->splat.
 * Honors BDPT_PARAM_NO_* flags.  counters may be NULL. */
int oracle_bdpt(const oracle_scene* s, const bdpt_camera* cam, const bdpt_params* p, oracle_frame* f,
                uint32_t flags, int threads, bdpt_counters* counters);

/* out = saturate(out + splat) where count != 0, rows [y0,y1). */
int oracle_resolve(oracle_frame* f);

void oracle_accumulate(float* lastFrame, float* curFrame, uint32_t accumCount, uint32_t maxAccumCount,
                       uint64_t numTexels);

/* Known-answer hooks mirroring bdpt_test_* of include/bdpt.h. */
void oracle_rng(const uint32_t* val0, const uint32_t* val1, uint32_t n, uint32_t draws, uint32_t* out_states,
                float* out_floats);
void oracle_trace(const oracle_scene* s, const float* rays, uint32_t n, int mode, uint32_t flags,
                  int32_t* out_prim, float* out_tuv);
void oracle_bsdf(const float* in, uint32_t n, uint32_t matIndex, float* out);
/* bdpt_shade_hits (include/bdpt.h "Surface queries") on host arrays: a loop over prepareShadingData with rays[i]'s origin as
 * the camera position, flags BDPT_SHADE_*, and the query's miss rule (prim < 0 or not a triangle of the scene). */
void oracle_shade_hits(const oracle_scene* s, const bdpt_ray* rays, const bdpt_hit* hits, uint32_t n, uint32_t flags,
                       bdpt_surface* out);
/* The any-hit alpha test of candidate i: triangle prim[i] (any triangle of the scene; the caller asks only about non-opaque
 * ones) at barycentrics uv[2i], uv[2i+1].  fails[i] = 1 where the candidate is ignored. */
void oracle_alpha_test(const oracle_scene* s, const uint32_t* prim, const float* uv, uint32_t n, uint8_t* fails);
/* Per-record hooks mirroring bdpt_light_query (BDPT_LIGHT_NEE, no emitter table, no hints) and bdpt_connect_query (both
 * modes) of include/bdpt.h: loops over the functions the frame's pixel loop calls, on the queries' input records, writing
 * the queries' output records (host memory).  lights: numLights >= 1 records.  seedsOut, the predecessors and the specular
 * bytes are optional, with the queries' meaning of NULL. */
void oracle_light_nee(const bdpt_light* lights, uint32_t numLights, const bdpt_surface* surfaces, const uint32_t* seeds, uint32_t n,
                      uint32_t matIndex, float minT, bdpt_light_sample* samples, uint32_t* seedsOut);
void oracle_connect_vertices(const bdpt_surface* eye, const bdpt_surface* light, const float* eyePrev, const float* lightPrev,
                             const uint8_t* eyeSpecular, const uint8_t* lightSpecular, uint32_t n, uint32_t matIndex, float minT,
                             bdpt_connect_sample* samples);
void oracle_connect_camera(const bdpt_camera* cam, uint32_t width, uint32_t height, const float* pixelJitter, const bdpt_surface* light,
                           const uint8_t* lightSpecular, uint32_t n, uint32_t matIndex, float minT, bdpt_camera_sample* samples);
void oracle_sincos2pi(const float* u, uint32_t n, float* s, float* c);
void oracle_half_round(const float* in, uint32_t n, float* out);

/* Area lights (BDPT_PARAM_AREA_LIGHTS, include/bdpt.h "Area lights"): oracle_bdpt honours the switch in p->flags (and
 * fails with MIS, as bdpt_execute does).  The emitter table is made from the positions the scene was created with.
 * The oracle cannot know which triangles the device build drops by alpha clipping: oracle_area_exclude lists them
 * (replacing an earlier list) and remakes the table; -1 on a NULL scene or an index out of range. */
int oracle_area_exclude(oracle_scene* s, const uint32_t* tris, uint32_t n);
/* bdpt_get_area_light_info of the oracle's table */
void oracle_area_light_info(const oracle_scene* s, bdpt_area_light_info* out);
/* The table: emitter count; each non-NULL array gets that many values (primitive, weight, area, CDF value). */
uint32_t oracle_area_table(const oracle_scene* s, uint32_t* prim, float* weight, float* area, float* cdf);
/* bdpt_test_area_light_sample on the oracle's table: modes 0 and 1, 16 floats per item (integers as bits). */
void oracle_area_light_sample(const oracle_scene* s, uint32_t mode, const uint32_t* states, const float* points, uint32_t n,
                              float* out);

/* BMFR denoise pass (bmfr_oracle.cpp; DenoisePass.cpp:146-279 + its three shaders).  Channels are
 * float4 per pixel; curNorm / albedo hold the half-precision G-buffer values widened to float. */
typedef struct oracle_bmfr oracle_bmfr;
oracle_bmfr* oracle_bmfr_create(uint32_t width, uint32_t height);
void oracle_bmfr_destroy(oracle_bmfr* b);
void oracle_bmfr_reset(oracle_bmfr* b);
int oracle_bmfr_execute(oracle_bmfr* b, const bdpt_bmfr_params* p, const float* curPos, const float* curNorm,
                        const float* albedo, float* noisy);
/* bdpt_bmfr_execute_motion: prevPos (float4 per pixel; null = oracle_bmfr_execute) is what preprocess reprojects and compares. */
int oracle_bmfr_execute_motion(oracle_bmfr* b, const bdpt_bmfr_params* p, const float* curPos, const float* curNorm,
                               const float* albedo, const float* prevPos, float* noisy);
/* Test hook: copies out BMFR_PrevNoisy (float4), the accept bools and prev_frame_pixel_f (float2); null skips one. */
void oracle_bmfr_state(const oracle_bmfr* b, float* prevNoisy, uint32_t* accept, float* prevPixel);

#ifdef __cplusplus
}
#endif
#endif
