// api_query.cpp — the per-item queries of the C ABI (include/bdpt.h): bdpt_trace_rays, bdpt_camera_rays, bdpt_shade_hits,
// bdpt_bsdf_query, bdpt_light_query, bdpt_connect_query, bdpt_splat_add, bdpt_walk_query, bdpt_ao_query, bdpt_gi_query,
// bdpt_direct_query, bdpt_env_query, bdpt_sky_query, bdpt_bsdf_pdf_query, bdpt_sky_mis_query, bdpt_ris_query, bdpt_reuse_query and bdpt_motion_query, on a
// caller's arrays in device memory, and bdpt_ao_execute, bdpt_gi_execute, bdpt_direct_execute, bdpt_sky_execute,
// bdpt_sky_mis_execute, bdpt_ris_execute, bdpt_ris_execute_reservoirs and bdpt_reuse_execute, the same kernels on the tile's G-buffer
// pixels.  Every one checks its arguments in a fixed order — the context's state (BDPT_E_STATE), then mode, flags and what goes together
// (BDPT_E_INVALID), then an empty call returns BDPT_OK, then the pointers — and a refused call enqueues nothing.  What is left goes through enqueueQuery.  None allocates or synchronises (but bdpt_light_query's
// first use of the emitter table), so all can be captured into a hipGraph.
#include <cstddef>
#include <initializer_list>
#include <string>

#include "api_common.hpp"

using namespace bdpt;

namespace {

bool frameSizeOk(uint32_t width, uint32_t height) { return width && height && (uint64_t)width * height < (1ull << 32); }

// The three pointers of a compacted ray list: `on` when any is set, and then `whole` (all three are: checked before an
// empty call returns) and `aligned` (checked with the other pointers).
struct CompactArgs {
  bool on, whole, aligned;
  CompactList list;
};
CompactArgs compactArgs(bdpt_ray* rays, uint32_t* items, uint32_t* count) {
  return {rays || items || count, rays && items && count, aligned(rays, 16) && aligned(items, 4) && aligned(count, 4),
          CompactList{reinterpret_cast<float4*>(rays), items, count}};
}
int needWholeCompact(bdpt_ctx* c, const char* what, const CompactArgs& k) {
  return !k.on || k.whole ? BDPT_OK : refuse(c, BDPT_E_INVALID, what, "compactRays, compactItems and compactCount go together");
}

// The accepted call: launch(st) on the caller's stream, ordered after the context's last call.
template <class Launch>
int enqueueQuery(bdpt_ctx* c, void* stream, Launch&& launch) {
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = orderAfterLast(c, st)) return rc;
  launch(st);
  HIPCHK(c, hipGetLastError());
  c->lastStream = st;
  return BDPT_OK;
}

const float4* f4(const void* p) { return reinterpret_cast<const float4*>(p); }
float4* f4(void* p) { return reinterpret_cast<float4*>(p); }

// What the five fused lighting calls share (ao, gi, direct, sky, sky_mis; the fields are device_item_source.hpp's).
int needFrame(bdpt_ctx* c, const char* what) {
  return c->frame.have ? BDPT_OK : refuse(c, BDPT_E_STATE, what, "no size (bdpt_resize first)");
}
// The pointers of an *_execute call: worldPosition, worldNormal, `out`, and the other half channels the call reads.
int checkGbuffer(bdpt_ctx* c, const char* what, const bdpt_gbuffer* gb, const float* out, bool diffuse, bool specRough) {
  if (aligned(gb->worldPosition, 16) && aligned(gb->worldNormal, 8) && (!diffuse || aligned(gb->materialDiffuse, 8)) &&
      (!specRough || aligned(gb->materialSpecRough, 8)) && aligned(out, 16))
    return BDPT_OK;
  const std::string why = std::string("worldPosition, worldNormal, ") + (diffuse ? "materialDiffuse, " : "") +
                          (specRough ? "materialSpecRough, " : "") + "or out missing or not aligned (16 bytes; the half channels 8)";
  return refuse(c, BDPT_E_INVALID, what, why.c_str());
}
// The pointers of a *_query call, each with its alignment (records and float4 results 16 bytes, words 4); an optional one
// may be null.  `names`: how the refusal lists them.
struct PtrArg { const void* p; uintptr_t align; bool optional = false; };
int checkRecords(bdpt_ctx* c, const char* what, const char* names, std::initializer_list<PtrArg> ptrs) {
  bool ok = true;
  for (const PtrArg& a : ptrs) ok = ok && ((a.optional && !a.p) || aligned(a.p, a.align));
  if (ok) return BDPT_OK;
  return refuse(c, BDPT_E_INVALID, what, (std::string(names) + " missing or not aligned (records 16 bytes, words 4)").c_str());
}
// The common fields of AoDev, GiDev, DirectDev, SkyDev or SkyMisDev: from a query descriptor (SEEDED: it has RNG states) ...
template <bool SEEDED, class Dev, class Desc>
void fillRecords(Dev& Q, const Desc* d) {
  Q.surf = f4(d->surfaces);
  Q.alive = d->alive;
  Q.range = {d->num, d->numDevice, d->minT};
  if constexpr (SEEDED) {
    Q.seeds = d->seeds;
    Q.seedsOut = d->seedsOut;
  }
}
// ... and from the tile's G-buffer pixels
template <class Dev>
void fillGbuffer(Dev& Q, const bdpt_ctx* c, const bdpt_gbuffer* gb, float* out, float minT) {
  Q.gbPosition = f4(gb->worldPosition);
  Q.gbNormal = gb->worldNormal;
  Q.pix = c->frame.P.pix;
  Q.out = f4(out);
  Q.range = {c->frame.P.Np, nullptr, minT};
}

}  // namespace

extern "C" {

static_assert(sizeof(bdpt_ray) == 32 && sizeof(bdpt_hit) == 16, "trace_rays_kernel reads a ray as two float4 and writes a hit as one");
int bdpt_trace_rays(bdpt_ctx* c, const bdpt_trace_desc* d, void* stream) {
  if (!c || !d) return BDPT_E_INVALID;
  if (int rc = needScene(c, "trace_rays")) return rc;
  if (d->mode > BDPT_TRACE_ANY) return refuse(c, BDPT_E_INVALID, "trace_rays", "unknown mode");
  if (!d->numRays) return BDPT_OK;
  if (!aligned(d->rays, 16) || (d->numRaysDevice && !aligned(d->numRaysDevice, 4)) ||
      (d->mode == BDPT_TRACE_ANY ? !d->visible : !aligned(d->hits, 16)))
    return refuse(c, BDPT_E_INVALID, "trace_rays", "rays, hits or visible missing or not aligned (rays and hits 16 bytes, numRaysDevice 4)");
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    launchTraceRays(c->scene.S, f4(d->rays), d->numRays, d->numRaysDevice, c->rayCursor, (int)d->mode, f4(d->hits), d->visible, c->grids,
                    c->numCUs, st);
  });
}

static_assert(sizeof(bdpt_surface) == 96 && sizeof(bdpt_bsdf_sample) == 32,
              "shade_hits_kernel writes a surface as six float4, bsdf_query_kernel a sample as two");
int bdpt_camera_rays(bdpt_ctx* c, const bdpt_gbuffer_params* p, uint32_t width, uint32_t height, bdpt_ray* rays, void* stream) {
  if (!c || !p) return BDPT_E_INVALID;
  if (int rc = needCamera(c, "camera_rays")) return rc;
  if (!frameSizeOk(width, height) || !aligned(rays, 16))
    return refuse(c, BDPT_E_INVALID, "camera_rays", "width and height must be > 0 with width * height < 2^32, rays 16-byte aligned");
  return enqueueQuery(c, stream, [&](hipStream_t st) { launchCameraRays(c->cam, *p, width, height, f4(rays), st); });
}

int bdpt_shade_hits(bdpt_ctx* c, const bdpt_shade_desc* d, void* stream) {
  if (!c || !d) return BDPT_E_INVALID;
  if (int rc = needScene(c, "shade_hits")) return rc;
  if (d->flags & ~BDPT_SHADE_NORMAL_MAP) return refuse(c, BDPT_E_INVALID, "shade_hits", "unknown flags");
  if (!d->numHits) return BDPT_OK;
  if (!aligned(d->rays, 16) || !aligned(d->hits, 16) || !aligned(d->surfaces, 16) || (d->numHitsDevice && !aligned(d->numHitsDevice, 4)))
    return refuse(c, BDPT_E_INVALID, "shade_hits", "rays, hits or surfaces missing or not aligned (16 bytes; numHitsDevice 4)");
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    launchShadeHits(c->scene.S, c->scene.numTriangles, f4(d->rays), f4(d->hits), d->numHits, d->numHitsDevice, (d->flags & BDPT_SHADE_NORMAL_MAP) != 0,
                    f4(d->surfaces), st);
  });
}

int bdpt_bsdf_query(bdpt_ctx* c, const bdpt_bsdf_desc* d, void* stream) {
  if (!c || !d) return BDPT_E_INVALID;
  if (int rc = needScene(c, "bsdf_query")) return rc;
  if (d->mode > BDPT_BSDF_EVAL || d->matIndex > 1 || (d->flags & ~BDPT_PARAM_SPECULAR_FROM_LOBE))
    return refuse(c, BDPT_E_INVALID, "bsdf_query", "unknown mode or flags, or matIndex > 1");
  if (!d->num) return BDPT_OK;
  const bool eval = d->mode == BDPT_BSDF_EVAL;
  if (!aligned(d->surfaces, 16) || (d->numDevice && !aligned(d->numDevice, 4)) ||
      (eval ? (!aligned(d->dirs, 16) || !aligned(d->values, 16)) : (!aligned(d->seeds, 4) || !aligned(d->samples, 16))))
    return refuse(c, BDPT_E_INVALID, "bsdf_query", "surfaces, seeds, samples, dirs or values missing or not aligned (16 bytes; seeds and numDevice 4)");
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    launchBsdfQuery(f4(d->surfaces), d->num, d->numDevice, eval, d->matIndex == 0, (d->flags & BDPT_PARAM_SPECULAR_FROM_LOBE) != 0, d->seeds,
                    f4(d->dirs), eval ? f4(d->values) : f4(d->samples), st);
  });
}

static_assert(sizeof(bdpt_light_sample) == 48 && sizeof(bdpt_light_emit) == 48 && offsetof(bdpt_light_sample, status) == 46,
              "the light query kernels write a record as three float4, light and status sharing the last word");
int bdpt_light_query(bdpt_ctx* c, const bdpt_light_desc* d, void* stream) {
  if (!c || !d) return BDPT_E_INVALID;
  if (int rc = needScene(c, "light_query")) return rc;
  const bool emitMode = d->mode == BDPT_LIGHT_EMIT;
  if (d->mode > BDPT_LIGHT_EMIT || d->matIndex > 1 || (d->flags & ~(BDPT_PARAM_AREA_LIGHTS | BDPT_LIGHT_USE_HINTS)))
    return refuse(c, BDPT_E_INVALID, "light_query", "unknown mode or flags, or matIndex > 1");
  const CompactArgs k = compactArgs(d->compactRays, d->compactItems, d->compactCount);
  if (emitMode && (k.on || (d->flags & BDPT_LIGHT_USE_HINTS)))
    return refuse(c, BDPT_E_INVALID, "light_query", "compaction and BDPT_LIGHT_USE_HINTS go with BDPT_LIGHT_NEE");
  if (int rc = needWholeCompact(c, "light_query", k)) return rc;
  if (!d->num) return BDPT_OK;
  if (!aligned(d->seeds, 4) || (d->seedsOut && !aligned(d->seedsOut, 4)) || (d->numDevice && !aligned(d->numDevice, 4)) ||
      (emitMode ? !aligned(d->emits, 16) : (!aligned(d->surfaces, 16) || !aligned(d->samples, 16))) || (k.on && !k.aligned))
    return refuse(c, BDPT_E_INVALID, "light_query",
                  "surfaces, seeds, samples, emits or a compaction buffer missing or not aligned (records 16 bytes, words 4)");
  AreaDev A{};
  // The table's first build synchronises the device, so it comes before enqueueQuery orders the call after the last one;
  // it needs the context's device current, hence an ENTER of its own (enqueueQuery's second one changes nothing).
  if (d->flags & BDPT_PARAM_AREA_LIGHTS) {
    ENTER(c);
    if (int rc = ensureAreaLights(c, reinterpret_cast<hipStream_t>(stream))) return rc;
    A = c->scene.area;  // n == 0 (no emitter): the plain instances
  }
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    LightQueryDev Q{};
    Q.surf = f4(d->surfaces);
    Q.seeds = d->seeds;
    Q.seedsOut = d->seedsOut;
    Q.out = emitMode ? f4(d->emits) : f4(d->samples);
    Q.range = {d->num, d->numDevice, d->minT};
    Q.compact = k.list;
    launchLightQuery(c->scene.S, Q, A, emitMode, d->matIndex == 0, (d->flags & BDPT_LIGHT_USE_HINTS) != 0, st);
  });
}

static_assert(sizeof(bdpt_connect_sample) == 48 && sizeof(bdpt_camera_sample) == 64 && offsetof(bdpt_connect_sample, status) == 44 &&
                  offsetof(bdpt_camera_sample, G) == 44 && offsetof(bdpt_camera_sample, pixel) == 48,
              "the connection query kernels write a record as three / four float4");
int bdpt_connect_query(bdpt_ctx* c, const bdpt_connect_desc* d, void* stream) {
  if (!c || !d) return BDPT_E_INVALID;
  if (int rc = needScene(c, "connect_query")) return rc;
  if (d->mode > BDPT_CONNECT_CAMERA || d->matIndex > 1 || d->flags || d->reserved)
    return refuse(c, BDPT_E_INVALID, "connect_query", "unknown mode, non-zero flags or reserved, or matIndex > 1");
  const bool camMode = d->mode == BDPT_CONNECT_CAMERA;
  if (camMode) {
    if (int rc = needCamera(c, "connect_query: BDPT_CONNECT_CAMERA")) return rc;
    if (!frameSizeOk(d->width, d->height))
      return refuse(c, BDPT_E_INVALID, "connect_query", "width and height must be > 0 with width * height < 2^32");
  }
  const CompactArgs k = compactArgs(d->compactRays, d->compactItems, d->compactCount);
  if (int rc = needWholeCompact(c, "connect_query", k)) return rc;
  if (!d->num) return BDPT_OK;
  if (!aligned(d->light, 16) || (d->numDevice && !aligned(d->numDevice, 4)) ||
      (camMode ? !aligned(d->cameraSamples, 16)
               : (!aligned(d->eye, 16) || !aligned(d->samples, 16) || (d->eyePrev && !aligned(d->eyePrev, 16)) ||
                  (d->lightPrev && !aligned(d->lightPrev, 16)))) ||
      (k.on && !k.aligned))
    return refuse(c, BDPT_E_INVALID, "connect_query",
                  "eye, light, samples, a predecessor or a compaction buffer missing or not aligned (records 16 bytes, words 4)");
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    ConnectQueryDev Q{};
    Q.light = f4(d->light);
    Q.lightSpecular = d->lightSpecular;
    if (camMode) {
      Q.out = f4(d->cameraSamples);
      Q.width = d->width;
      Q.height = d->height;
      Q.jitter[0] = d->pixelJitter[0];
      Q.jitter[1] = d->pixelJitter[1];
    } else {
      Q.eye = f4(d->eye);
      Q.eyePrev = f4(d->eyePrev);
      Q.lightPrev = f4(d->lightPrev);
      Q.eyeSpecular = d->eyeSpecular;
      Q.out = f4(d->samples);
    }
    Q.range = {d->num, d->numDevice, d->minT};
    Q.compact = k.list;
    launchConnectQuery(Q, camMode ? &c->cam : nullptr, d->matIndex == 0, st);
  });
}

int bdpt_splat_add(bdpt_ctx* c, const bdpt_splat_desc* d, void* stream) {
  if (!c || !d) return BDPT_E_INVALID;
  if (!d->num) return BDPT_OK;
  if (!aligned(d->pixels, 4) || !aligned(d->values, 16) || !aligned(d->splat, 16) || (d->items && !aligned(d->items, 4)) ||
      (d->numDevice && !aligned(d->numDevice, 4)))
    return refuse(c, BDPT_E_INVALID, "splat_add", "pixels, values, splat, items or numDevice missing or not aligned (splat and values 16 bytes, words 4)");
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    SplatAddDev A{};
    A.pixels = d->pixels;
    A.values = f4(d->values);
    A.visible = d->visible;
    A.items = d->items;
    A.splat = reinterpret_cast<unsigned long long*>(d->splat);
    A.numPixels = d->numPixels;
    A.cap = d->num;
    A.count = d->numDevice;
    launchSplatAdd(A, st);
  });
}

static_assert(sizeof(bdpt_walk_start) == 48 && sizeof(bdpt_walk_start) == sizeof(bdpt_light_emit) &&
                  offsetof(bdpt_walk_start, color) == offsetof(bdpt_light_emit, color) && sizeof(bdpt_walk_info) == 16 &&
                  offsetof(bdpt_walk_info, status) == 12,
              "walk_query_kernel reads a start as three float4 (bdpt_light_emit's layout) and writes an info record as one");
int bdpt_walk_query(bdpt_ctx* c, const bdpt_walk_desc* d, void* stream) {
  if (!c || !d) return BDPT_E_INVALID;
  if (int rc = needScene(c, "walk_query")) return rc;
  if (!d->steps || d->steps > BDPT_MAX_DEPTH || d->matIndex > 1 || (d->flags & ~(BDPT_PARAM_SPECULAR_FROM_LOBE | BDPT_WALK_SEED_PER_STEP)) ||
      d->reserved || (uint64_t)d->steps * d->num >= (1ull << 32))
    return refuse(c, BDPT_E_INVALID, "walk_query",
                  "steps outside 1 .. BDPT_MAX_DEPTH, matIndex > 1, unknown flags, non-zero reserved, or steps * num >= 2^32");
  if (!d->num) return BDPT_OK;
  if (!aligned(d->starts, 16) || !aligned(d->seeds, 4) || !aligned(d->vertices, 16) || !aligned(d->info, 16) ||
      (d->first && !aligned(d->first, 16)) || (d->samples && !aligned(d->samples, 16)) || (d->hits && !aligned(d->hits, 16)) ||
      (d->numDevice && !aligned(d->numDevice, 4)))
    return refuse(c, BDPT_E_INVALID, "walk_query",
                  "starts, seeds, vertices, info, first, samples or hits missing or not aligned (records 16 bytes, words 4)");
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    WalkQueryDev Q{};
    Q.starts = f4(d->starts);
    Q.seeds = d->seeds;
    Q.first = f4(d->first);
    Q.firstSpecular = d->firstSpecular;
    Q.alive = d->alive;
    Q.vertices = f4(d->vertices);
    Q.info = f4(d->info);
    Q.samples = f4(d->samples);
    Q.hits = f4(d->hits);
    Q.range = {d->num, d->numDevice, d->minT};
    Q.steps = d->steps;
    Q.seedPerStep = (d->flags & BDPT_WALK_SEED_PER_STEP) ? 1u : 0u;
    launchWalkQuery(c->scene.S, Q, d->matIndex == 0, (d->flags & BDPT_PARAM_SPECULAR_FROM_LOBE) != 0, c->rayCursor, c->grids, c->numCUs, st);
  });
}

int bdpt_ao_query(bdpt_ctx* c, const bdpt_ao_desc* d, void* stream) {
  if (!c || !d) return BDPT_E_INVALID;
  if (int rc = needScene(c, "ao_query")) return rc;
  if (!d->samples || d->samples > BDPT_AO_MAX_SAMPLES || d->flags || d->reserved)
    return refuse(c, BDPT_E_INVALID, "ao_query", "samples outside 1 .. BDPT_AO_MAX_SAMPLES, or non-zero flags or reserved");
  if (!d->num) return BDPT_OK;
  if (int rc = checkRecords(c, "ao_query", "surfaces, seeds, ao, counts, seedsOut or numDevice",
                            {{d->surfaces, 16}, {d->seeds, 4}, {d->ao, 4}, {d->counts, 4, true}, {d->seedsOut, 4, true}, {d->numDevice, 4, true}}))
    return rc;
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    AoDev A{};
    fillRecords<true>(A, d);
    A.ao = d->ao;
    A.counts = d->counts;
    A.radius = d->radius;
    A.samples = d->samples;
    launchAo(c->scene.S, A, false, c->rayCursor, c->grids, c->numCUs, st);
  });
}

int bdpt_ao_execute(bdpt_ctx* c, const bdpt_ao_params* p, const bdpt_gbuffer* gb, float* out, void* stream) {
  if (!c || !p || !gb) return BDPT_E_INVALID;
  if (int rc = needScene(c, "ao_execute")) return rc;
  if (int rc = needFrame(c, "ao_execute")) return rc;
  if (!p->samples || p->samples > BDPT_AO_MAX_SAMPLES || p->reserved)
    return refuse(c, BDPT_E_INVALID, "ao_execute", "samples outside 1 .. BDPT_AO_MAX_SAMPLES, or non-zero reserved");
  if (int rc = checkGbuffer(c, "ao_execute", gb, out, false, false)) return rc;
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    AoDev A{};
    fillGbuffer(A, c, gb, out, p->minT);
    A.radius = p->radius;
    A.samples = p->samples;
    A.frameCount = p->frameCount;
    launchAo(c->scene.S, A, true, c->rayCursor, c->grids, c->numCUs, st);
  });
}

namespace {
// the context's environment (bdpt_set_environment), as the walk's miss branch reads it
void giEnvironment(const bdpt_ctx* c, GiDev& Q) {
  Q.envMap = c->env.envMap;
  Q.envW = c->env.width;
  Q.envH = c->env.height;
  for (int k = 0; k < 3; k++) Q.envColor[k] = c->env.color[k];
}
}  // namespace

static_assert(sizeof(bdpt_gi_desc) == 96 && offsetof(bdpt_gi_desc, surfaces) == 40 && sizeof(bdpt_gi_params) == 16,
              "abi.GiDesc and abi.GiParams restate these layouts");
int bdpt_gi_query(bdpt_ctx* c, const bdpt_gi_desc* d, void* stream) {
  if (!c || !d) return BDPT_E_INVALID;
  if (int rc = needScene(c, "gi_query")) return rc;
  if ((d->flags & ~(BDPT_GI_INDIRECT | BDPT_GI_UNIFORM | BDPT_GI_SHADE_FROM_VIEW)) || (d->shadeFlags & ~BDPT_SHADE_NORMAL_MAP) || d->reserved)
    return refuse(c, BDPT_E_INVALID, "gi_query", "unknown flags or shadeFlags, or non-zero reserved");
  if (!d->num) return BDPT_OK;
  if (int rc = checkRecords(c, "gi_query", "surfaces, seeds, color, hits, status, seedsOut or numDevice",
                            {{d->surfaces, 16}, {d->seeds, 4}, {d->color, 16}, {d->hits, 16, true}, {d->status, 4, true},
                             {d->seedsOut, 4, true}, {d->numDevice, 4, true}}))
    return rc;
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    GiDev Q{};
    fillRecords<true>(Q, d);
    Q.color = f4(d->color);
    Q.hits = f4(d->hits);
    Q.status = d->status;
    Q.flags = d->flags;
    for (int k = 0; k < 3; k++) Q.viewPos[k] = d->viewPos[k];
    giEnvironment(c, Q);
    launchGi(c->scene.S, Q, false, (d->shadeFlags & BDPT_SHADE_NORMAL_MAP) != 0, c->rayCursor, c->grids, c->numCUs, st);
  });
}

int bdpt_gi_execute(bdpt_ctx* c, const bdpt_gi_params* p, const bdpt_gbuffer* gb, float* out, void* stream) {
  if (!c || !p || !gb) return BDPT_E_INVALID;
  if (int rc = needScene(c, "gi_execute")) return rc;
  if (int rc = needFrame(c, "gi_execute")) return rc;
  if (int rc = needCamera(c, "gi_execute")) return rc;
  if ((p->flags & ~(BDPT_GI_INDIRECT | BDPT_GI_UNIFORM)) || p->reserved)
    return refuse(c, BDPT_E_INVALID, "gi_execute", "flags other than BDPT_GI_INDIRECT | BDPT_GI_UNIFORM, or non-zero reserved");
  if (int rc = checkGbuffer(c, "gi_execute", gb, out, true, false)) return rc;
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    GiDev Q{};
    fillGbuffer(Q, c, gb, out, p->minT);
    Q.gbDiffuse = gb->materialDiffuse;
    Q.flags = p->flags | BDPT_GI_SHADE_FROM_VIEW;  // prepareShadingData shades from gCamera.posW
    Q.frameCount = p->frameCount;
    for (int k = 0; k < 3; k++) Q.viewPos[k] = c->cam.posW[k];
    giEnvironment(c, Q);
    launchGi(c->scene.S, Q, true, true, c->rayCursor, c->grids, c->numCUs, st);
  });
}

static_assert(sizeof(bdpt_direct_desc) == 64 && offsetof(bdpt_direct_desc, surfaces) == 24 && sizeof(bdpt_direct_params) == 16,
              "abi.DirectDesc and abi.DirectParams restate these layouts");
int bdpt_direct_query(bdpt_ctx* c, const bdpt_direct_desc* d, void* stream) {
  if (!c || !d) return BDPT_E_INVALID;
  if (int rc = needScene(c, "direct_query")) return rc;
  if ((d->flags & ~BDPT_DIRECT_USE_HINTS) || d->reserved)
    return refuse(c, BDPT_E_INVALID, "direct_query",
                  "flags other than BDPT_DIRECT_USE_HINTS (the emitter table is not part of this call), or non-zero reserved");
  if (!d->num) return BDPT_OK;
  if (int rc = checkRecords(c, "direct_query", "surfaces, color, visible, traced or numDevice",
                            {{d->surfaces, 16}, {d->color, 16}, {d->visible, 4, true}, {d->traced, 4, true}, {d->numDevice, 4, true}}))
    return rc;
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    DirectDev Q{};
    fillRecords<false>(Q, d);
    Q.color = f4(d->color);
    Q.visible = d->visible;
    Q.traced = d->traced;
    launchDirect(c->scene.S, Q, false, (d->flags & BDPT_DIRECT_USE_HINTS) != 0, c->rayCursor, c->grids, c->numCUs, st);
  });
}

int bdpt_direct_execute(bdpt_ctx* c, const bdpt_direct_params* p, const bdpt_gbuffer* gb, float* out, void* stream) {
  if (!c || !p || !gb) return BDPT_E_INVALID;
  if (int rc = needScene(c, "direct_execute")) return rc;
  if (int rc = needFrame(c, "direct_execute")) return rc;
  if ((p->flags & ~BDPT_DIRECT_USE_HINTS) || p->reserved[0] || p->reserved[1])
    return refuse(c, BDPT_E_INVALID, "direct_execute",
                  "flags other than BDPT_DIRECT_USE_HINTS (the emitter table is not part of this call), or non-zero reserved");
  if (int rc = checkGbuffer(c, "direct_execute", gb, out, true, true)) return rc;
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    DirectDev Q{};
    fillGbuffer(Q, c, gb, out, p->minT);
    Q.gbDiffuse = gb->materialDiffuse;
    Q.gbSpecRough = gb->materialSpecRough;
    launchDirect(c->scene.S, Q, true, (p->flags & BDPT_DIRECT_USE_HINTS) != 0, c->rayCursor, c->grids, c->numCUs, st);
  });
}

namespace {
int needEnvTable(bdpt_ctx* c, const char* what) {
  if (c->envTable.ready) return BDPT_OK;
  return refuse(c, BDPT_E_STATE, what,
                c->env.envMap ? "no sampling table for the environment map (bdpt_env_prepare first, and again after bdpt_set_environment)"
                              : "no environment map (bdpt_set_environment with a map, then bdpt_env_prepare)");
}
}  // namespace

static_assert(sizeof(bdpt_env_sample) == 80 && offsetof(bdpt_env_sample, radiance) == 32 && offsetof(bdpt_env_sample, value) == 48 &&
                  offsetof(bdpt_env_sample, texel) == 60 && offsetof(bdpt_env_sample, status) == 64 && sizeof(bdpt_env_eval) == 32 &&
                  offsetof(bdpt_env_eval, texel) == 16,
              "the environment query kernels write a sample as five float4 and an evaluation as two");
static_assert(sizeof(bdpt_env_desc) == 104 && sizeof(bdpt_env_info) == 56 && sizeof(bdpt_sky_desc) == 80 && sizeof(bdpt_sky_params) == 20,
              "abi.EnvDesc, abi.EnvInfo, abi.SkyDesc and abi.SkyParams restate these layouts");
int bdpt_env_query(bdpt_ctx* c, const bdpt_env_desc* d, void* stream) {
  if (!c || !d) return BDPT_E_INVALID;
  if (int rc = needEnvTable(c, "env_query")) return rc;
  const bool evalMode = d->mode == BDPT_ENV_EVAL;
  if (d->mode > BDPT_ENV_EVAL || d->matIndex > 1 || d->flags || d->reserved)
    return refuse(c, BDPT_E_INVALID, "env_query", "unknown mode, non-zero flags or reserved, or matIndex > 1");
  const CompactArgs k = compactArgs(d->compactRays, d->compactItems, d->compactCount);
  if (evalMode && k.on) return refuse(c, BDPT_E_INVALID, "env_query", "compaction goes with BDPT_ENV_SAMPLE");
  if (int rc = needWholeCompact(c, "env_query", k)) return rc;
  if (!d->num) return BDPT_OK;
  if ((d->numDevice && !aligned(d->numDevice, 4)) ||
      (evalMode ? (!aligned(d->dirs, 16) || !aligned(d->evals, 16))
                : (!aligned(d->surfaces, 16) || !aligned(d->seeds, 4) || !aligned(d->samples, 16) || (d->seedsOut && !aligned(d->seedsOut, 4)))) ||
      (k.on && !k.aligned))
    return refuse(c, BDPT_E_INVALID, "env_query",
                  "surfaces, seeds, samples, dirs, evals or a compaction buffer missing or not aligned (records 16 bytes, words 4)");
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    EnvQueryDev Q{};
    Q.table = c->envTable.table;
    Q.surf = f4(d->surfaces);
    Q.seeds = d->seeds;
    Q.seedsOut = d->seedsOut;
    Q.dirs = f4(d->dirs);
    Q.out = evalMode ? f4(d->evals) : f4(d->samples);
    Q.range = {d->num, d->numDevice, d->minT};
    Q.compact = k.list;
    launchEnvQuery(Q, evalMode, d->matIndex == 0, st);
  });
}

int bdpt_sky_query(bdpt_ctx* c, const bdpt_sky_desc* d, void* stream) {
  if (!c || !d) return BDPT_E_INVALID;
  if (int rc = needScene(c, "sky_query")) return rc;
  if (int rc = needEnvTable(c, "sky_query")) return rc;
  if (!d->samples || d->samples > BDPT_SKY_MAX_SAMPLES || d->flags || d->reserved)
    return refuse(c, BDPT_E_INVALID, "sky_query", "samples outside 1 .. BDPT_SKY_MAX_SAMPLES, or non-zero flags or reserved");
  if (!d->num) return BDPT_OK;
  if (int rc = checkRecords(c, "sky_query", "surfaces, seeds, color, counts, seedsOut or numDevice",
                            {{d->surfaces, 16}, {d->seeds, 4}, {d->color, 16}, {d->counts, 4, true}, {d->seedsOut, 4, true}, {d->numDevice, 4, true}}))
    return rc;
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    SkyDev Q{};
    Q.table = c->envTable.table;
    fillRecords<true>(Q, d);
    Q.color = f4(d->color);
    Q.counts = d->counts;
    Q.clampUpper = d->clampUpper;
    Q.samples = d->samples;
    launchSky(c->scene.S, Q, false, c->rayCursor, c->grids, c->numCUs, st);
  });
}

int bdpt_sky_execute(bdpt_ctx* c, const bdpt_sky_params* p, const bdpt_gbuffer* gb, float* out, void* stream) {
  if (!c || !p || !gb) return BDPT_E_INVALID;
  if (int rc = needScene(c, "sky_execute")) return rc;
  if (int rc = needFrame(c, "sky_execute")) return rc;
  if (int rc = needEnvTable(c, "sky_execute")) return rc;
  if (!p->samples || p->samples > BDPT_SKY_MAX_SAMPLES || p->reserved)
    return refuse(c, BDPT_E_INVALID, "sky_execute", "samples outside 1 .. BDPT_SKY_MAX_SAMPLES, or non-zero reserved");
  if (int rc = checkGbuffer(c, "sky_execute", gb, out, true, false)) return rc;
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    SkyDev Q{};
    Q.table = c->envTable.table;
    fillGbuffer(Q, c, gb, out, p->minT);
    Q.gbDiffuse = gb->materialDiffuse;
    Q.clampUpper = p->clampUpper;
    Q.samples = p->samples;
    Q.frameCount = p->frameCount;
    launchSky(c->scene.S, Q, true, c->rayCursor, c->grids, c->numCUs, st);
  });
}

static_assert(sizeof(bdpt_bsdf_pdf_desc) == 48 && offsetof(bdpt_bsdf_pdf_desc, surfaces) == 24 && sizeof(bdpt_sky_mis_desc) == 88 &&
                  offsetof(bdpt_sky_mis_desc, surfaces) == 40 && sizeof(bdpt_sky_mis_params) == 32,
              "abi.BsdfPdfDesc, abi.SkyMisDesc and abi.SkyMisParams restate these layouts");
int bdpt_bsdf_pdf_query(bdpt_ctx* c, const bdpt_bsdf_pdf_desc* d, void* stream) {
  if (!c || !d) return BDPT_E_INVALID;
  if (int rc = needScene(c, "bsdf_pdf_query")) return rc;
  if (d->matIndex > 1 || d->flags || d->reserved)
    return refuse(c, BDPT_E_INVALID, "bsdf_pdf_query", "matIndex > 1, or non-zero flags or reserved");
  if (!d->num) return BDPT_OK;
  if (!aligned(d->surfaces, 16) || !aligned(d->dirs, 16) || !aligned(d->values, 16) || (d->numDevice && !aligned(d->numDevice, 4)))
    return refuse(c, BDPT_E_INVALID, "bsdf_pdf_query", "surfaces, dirs or values missing or not aligned (16 bytes; numDevice 4)");
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    launchBsdfPdfQuery(f4(d->surfaces), d->num, d->numDevice, d->matIndex == 0, f4(d->dirs), f4(d->values), st);
  });
}

namespace {
bool skyMisModeOk(uint32_t samples, uint32_t matIndex, uint32_t techniques) {
  return samples && samples <= BDPT_SKY_MAX_SAMPLES && matIndex <= 1 && techniques >= 1 && techniques <= 3;
}
}  // namespace

int bdpt_sky_mis_query(bdpt_ctx* c, const bdpt_sky_mis_desc* d, void* stream) {
  if (!c || !d) return BDPT_E_INVALID;
  if (int rc = needScene(c, "sky_mis_query")) return rc;
  if (int rc = needEnvTable(c, "sky_mis_query")) return rc;
  if (!skyMisModeOk(d->samples, d->matIndex, d->techniques) || d->flags || d->reserved)
    return refuse(c, BDPT_E_INVALID, "sky_mis_query",
                  "samples outside 1 .. BDPT_SKY_MAX_SAMPLES, matIndex > 1, techniques outside 1 .. 3, or non-zero flags or reserved");
  if (!d->num) return BDPT_OK;
  if (int rc = checkRecords(c, "sky_mis_query", "surfaces, seeds, color, counts, seedsOut or numDevice",
                            {{d->surfaces, 16}, {d->seeds, 4}, {d->color, 16}, {d->counts, 4, true}, {d->seedsOut, 4, true}, {d->numDevice, 4, true}}))
    return rc;
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    SkyMisDev Q{};
    Q.table = c->envTable.table;
    fillRecords<true>(Q, d);
    Q.color = f4(d->color);
    Q.counts = d->counts;
    Q.clampUpper = d->clampUpper;
    Q.samples = d->samples;
    Q.techniques = d->techniques;
    launchSkyMis(c->scene.S, Q, false, d->matIndex == 0, c->rayCursor, c->grids, c->numCUs, st);
  });
}

int bdpt_sky_mis_execute(bdpt_ctx* c, const bdpt_sky_mis_params* p, const bdpt_gbuffer* gb, float* out, void* stream) {
  if (!c || !p || !gb) return BDPT_E_INVALID;
  if (int rc = needScene(c, "sky_mis_execute")) return rc;
  if (int rc = needFrame(c, "sky_mis_execute")) return rc;
  if (int rc = needEnvTable(c, "sky_mis_execute")) return rc;
  const bool ggx = p->matIndex == 0;  // V comes from the camera
  if (ggx)
    if (int rc = needCamera(c, "sky_mis_execute: matIndex 0")) return rc;
  if (!skyMisModeOk(p->samples, p->matIndex, p->techniques) || p->reserved[0] || p->reserved[1])
    return refuse(c, BDPT_E_INVALID, "sky_mis_execute",
                  "samples outside 1 .. BDPT_SKY_MAX_SAMPLES, matIndex > 1, techniques outside 1 .. 3, or non-zero reserved");
  if (int rc = checkGbuffer(c, "sky_mis_execute", gb, out, true, ggx)) return rc;
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    SkyMisDev Q{};
    Q.table = c->envTable.table;
    fillGbuffer(Q, c, gb, out, p->minT);
    Q.gbDiffuse = gb->materialDiffuse;
    Q.gbSpecRough = gb->materialSpecRough;
    if (ggx)
      for (int k = 0; k < 3; k++) Q.camPos[k] = c->cam.posW[k];
    Q.clampUpper = p->clampUpper;
    Q.samples = p->samples;
    Q.techniques = p->techniques;
    Q.frameCount = p->frameCount;
    launchSkyMis(c->scene.S, Q, true, ggx, c->rayCursor, c->grids, c->numCUs, st);
  });
}

namespace {
bool risModeOk(uint32_t candidates, uint32_t samples, uint32_t matIndex, uint32_t flags, float clampUpper) {
  return candidates && candidates <= BDPT_RIS_MAX_CANDIDATES && samples && samples <= BDPT_RIS_MAX_SAMPLES && matIndex <= 1 &&
         !(flags & ~(BDPT_PARAM_AREA_LIGHTS | BDPT_RIS_USE_HINTS)) && clampUpper >= 0.0f;  // (a NaN fails the comparison)
}
const char* const kRisModeWhy =
    "candidates outside 1 .. BDPT_RIS_MAX_CANDIDATES, samples outside 1 .. BDPT_RIS_MAX_SAMPLES, matIndex > 1, unknown flags, "
    "non-zero reserved, or a negative or NaN clampUpper";
// The emitter table of a call with BDPT_PARAM_AREA_LIGHTS, as bdpt_light_query takes it: the first build synchronises the
// device, so it comes before enqueueQuery, under an ENTER of its own.  n == 0 (no emitter): the plain instances.
int risArea(bdpt_ctx* c, uint32_t flags, void* stream, AreaDev& A) {
  A = AreaDev{};
  if (!(flags & BDPT_PARAM_AREA_LIGHTS)) return BDPT_OK;
  ENTER(c);
  if (int rc = ensureAreaLights(c, reinterpret_cast<hipStream_t>(stream))) return rc;
  A = c->scene.area;
  return BDPT_OK;
}
}  // namespace

static_assert(sizeof(bdpt_ris_desc) == 96 && offsetof(bdpt_ris_desc, surfaces) == 40 && sizeof(bdpt_ris_params) == 32 &&
                  sizeof(bdpt_ris_reservoir) == 16 && offsetof(bdpt_ris_reservoir, status) == 2,
              "abi.RisDesc and abi.RisParams restate these layouts; ris_kernel writes a reservoir as one uint4");
int bdpt_ris_query(bdpt_ctx* c, const bdpt_ris_desc* d, void* stream) {
  if (!c || !d) return BDPT_E_INVALID;
  if (int rc = needScene(c, "ris_query")) return rc;
  if (!risModeOk(d->candidates, d->samples, d->matIndex, d->flags, d->clampUpper) || d->reserved)
    return refuse(c, BDPT_E_INVALID, "ris_query", kRisModeWhy);
  if (!d->num) return BDPT_OK;
  if (int rc = checkRecords(c, "ris_query", "surfaces, seeds, color, seedsOut, traced, reservoirs or numDevice",
                            {{d->surfaces, 16}, {d->seeds, 4}, {d->color, 16}, {d->seedsOut, 4, true}, {d->traced, 4, true},
                             {d->reservoirs, 16, true}, {d->numDevice, 4, true}}))
    return rc;
  AreaDev A;
  if (int rc = risArea(c, d->flags, stream, A)) return rc;
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    RisDev Q{};
    fillRecords<true>(Q, d);
    Q.color = f4(d->color);
    Q.traced = d->traced;
    Q.reservoirs = reinterpret_cast<uint4*>(d->reservoirs);
    Q.clampUpper = d->clampUpper;
    Q.candidates = d->candidates;
    Q.samples = d->samples;
    launchRis(c->scene.S, Q, A, false, d->matIndex == 0, (d->flags & BDPT_RIS_USE_HINTS) != 0, c->rayCursor, c->grids, c->numCUs, st);
  });
}

namespace {
// bdpt_ris_execute, and with wantReservoirs bdpt_ris_execute_reservoirs: the full-frame reservoir image beside `out`
int risExecute(bdpt_ctx* c, const bdpt_ris_params* p, const bdpt_gbuffer* gb, float* out, bdpt_ris_reservoir* reservoirs, bool wantReservoirs,
               void* stream) {
  if (!c || !p || !gb) return BDPT_E_INVALID;
  if (int rc = needScene(c, "ris_execute")) return rc;
  if (int rc = needFrame(c, "ris_execute")) return rc;
  const bool ggx = p->matIndex == 0;  // V comes from the camera
  if (ggx)
    if (int rc = needCamera(c, "ris_execute: matIndex 0")) return rc;
  if (!risModeOk(p->candidates, p->samples, p->matIndex, p->flags, p->clampUpper) || p->reserved)
    return refuse(c, BDPT_E_INVALID, "ris_execute", kRisModeWhy);
  if (int rc = checkGbuffer(c, "ris_execute", gb, out, true, ggx)) return rc;
  if (wantReservoirs && !aligned(reservoirs, 16))
    return refuse(c, BDPT_E_INVALID, "ris_execute_reservoirs", "reservoirs missing or not aligned (16 bytes)");
  AreaDev A;
  if (int rc = risArea(c, p->flags, stream, A)) return rc;
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    RisDev Q{};
    fillGbuffer(Q, c, gb, out, p->minT);
    Q.reservoirs = reinterpret_cast<uint4*>(reservoirs);
    Q.gbDiffuse = gb->materialDiffuse;
    Q.gbSpecRough = gb->materialSpecRough;
    if (ggx)
      for (int k = 0; k < 3; k++) Q.camPos[k] = c->cam.posW[k];
    Q.clampUpper = p->clampUpper;
    Q.candidates = p->candidates;
    Q.samples = p->samples;
    Q.frameCount = p->frameCount;
    launchRis(c->scene.S, Q, A, true, ggx, (p->flags & BDPT_RIS_USE_HINTS) != 0, c->rayCursor, c->grids, c->numCUs, st);
  });
}
}  // namespace
int bdpt_ris_execute(bdpt_ctx* c, const bdpt_ris_params* p, const bdpt_gbuffer* gb, float* out, void* stream) {
  return risExecute(c, p, gb, out, nullptr, false, stream);
}
int bdpt_ris_execute_reservoirs(bdpt_ctx* c, const bdpt_ris_params* p, const bdpt_gbuffer* gb, float* out, bdpt_ris_reservoir* reservoirs,
                                void* stream) {
  return risExecute(c, p, gb, out, reservoirs, true, stream);
}

static_assert(sizeof(bdpt_reuse_desc) == 160 && offsetof(bdpt_reuse_desc, surfaces) == 64 && sizeof(bdpt_reuse_reservoir) == 16 &&
                  offsetof(bdpt_reuse_reservoir, M) == 12,
              "abi.ReuseDesc restates this layout; reuse_kernel reads and writes a reservoir as one uint4");
namespace {
bool reuseModeOk(uint32_t neighbors, uint32_t matIndex, float clampUpper) {
  return neighbors <= BDPT_REUSE_MAX_NEIGHBORS && matIndex <= 1 && clampUpper >= 0.0f;  // (a NaN fails the comparison)
}
const char* const kReuseModeWhy =
    "neighbors > BDPT_REUSE_MAX_NEIGHBORS, matIndex > 1, unknown flags, non-zero reserved, or a negative or NaN clampUpper";
}  // namespace
int bdpt_reuse_query(bdpt_ctx* c, const bdpt_reuse_desc* d, void* stream) {
  if (!c || !d) return BDPT_E_INVALID;
  if (int rc = needScene(c, "reuse_query")) return rc;
  if (!reuseModeOk(d->neighbors, d->matIndex, d->clampUpper) || (d->flags & ~BDPT_PARAM_AREA_LIGHTS) || d->reserved[0] || d->reserved[1])
    return refuse(c, BDPT_E_INVALID, "reuse_query", kReuseModeWhy);
  if (!d->num) return BDPT_OK;
  const bool pooled = d->neighbors && d->poolNum;  // without either no pool entry is read
  if (int rc = checkRecords(c, "reuse_query", "surfaces, seeds, in, poolSurfaces, pool, neighborIndex, color, seedsOut, traced, out or numDevice",
                            {{d->surfaces, 16}, {d->seeds, 4}, {d->in, 16}, {d->poolSurfaces, 16, !pooled}, {d->pool, 16, !pooled},
                             {d->neighborIndex, 4, !d->neighbors}, {d->color, 16}, {d->seedsOut, 4, true}, {d->traced, 4, true},
                             {d->out, 16, true}, {d->numDevice, 4, true}}))
    return rc;
  if (d->out && (d->out == d->in || d->out == d->pool))
    return refuse(c, BDPT_E_INVALID, "reuse_query", "out must not be in or pool: other items read those records");
  AreaDev A;
  if (int rc = risArea(c, d->flags, stream, A)) return rc;
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    ReuseDev Q{};
    fillRecords<true>(Q, d);
    Q.color = f4(d->color);
    Q.traced = d->traced;
    Q.in = reinterpret_cast<const uint4*>(d->in);
    Q.res = reinterpret_cast<uint4*>(d->out);
    Q.poolSurf = f4(d->poolSurfaces);
    Q.poolAlive = d->poolAlive;
    Q.pool = reinterpret_cast<const uint4*>(d->pool);
    Q.neighborIndex = d->neighborIndex;
    Q.poolNum = pooled ? d->poolNum : 0u;
    Q.neighbors = d->neighbors;
    Q.inM = d->inM;
    Q.poolM = d->poolM;
    Q.maxM = d->maxM;
    Q.normalMin = d->normalMin;
    Q.planeMax = d->planeMax;
    Q.clampUpper = d->clampUpper;
    launchReuse(c->scene.S, Q, A, false, d->matIndex == 0, c->rayCursor, c->grids, c->numCUs, st);
  });
}

static_assert(sizeof(bdpt_reuse_params) == 104 && offsetof(bdpt_reuse_params, in) == 64, "abi.ReuseParams restates this layout");
int bdpt_reuse_execute(bdpt_ctx* c, const bdpt_reuse_params* p, const bdpt_gbuffer* gb, float* out, void* stream) {
  if (!c || !p || !gb) return BDPT_E_INVALID;
  if (int rc = needScene(c, "reuse_execute")) return rc;
  if (int rc = needFrame(c, "reuse_execute")) return rc;
  const bool ggx = p->matIndex == 0;  // V comes from the camera
  if (ggx)
    if (int rc = needCamera(c, "reuse_execute: matIndex 0")) return rc;
  if (!reuseModeOk(p->neighbors, p->matIndex, p->clampUpper) || (p->flags & ~(BDPT_PARAM_AREA_LIGHTS | BDPT_REUSE_SAME_PIXEL)) || p->reserved)
    return refuse(c, BDPT_E_INVALID, "reuse_execute", kReuseModeWhy);
  const bool same = (p->flags & BDPT_REUSE_SAME_PIXEL) != 0;
  const bool drawn = p->neighbors && !same && !p->neighborIndex;
  if ((same && (p->neighborIndex || p->neighbors != 1)) || (drawn && (p->radius < 1 || p->radius > BDPT_REUSE_MAX_RADIUS)))
    return refuse(c, BDPT_E_INVALID, "reuse_execute",
                  "neighbours come from one source: neighborIndex, BDPT_REUSE_SAME_PIXEL with neighbors 1, or a radius in 1 .. BDPT_REUSE_MAX_RADIUS");
  if (int rc = checkGbuffer(c, "reuse_execute", gb, out, true, ggx)) return rc;
  if (p->neighbors) {
    if (!p->poolGbuffer) return refuse(c, BDPT_E_INVALID, "reuse_execute", "poolGbuffer missing");
    if (int rc = checkGbuffer(c, "reuse_execute: poolGbuffer", p->poolGbuffer, out, true, ggx)) return rc;
  }
  if (int rc = checkRecords(c, "reuse_execute", "in, pool, neighborIndex or outReservoirs",
                            {{p->in, 16}, {p->pool, 16, !p->neighbors}, {p->neighborIndex, 4, true}, {p->outReservoirs, 16, true}}))
    return rc;
  if (p->outReservoirs && (p->outReservoirs == p->in || p->outReservoirs == p->pool))
    return refuse(c, BDPT_E_INVALID, "reuse_execute", "outReservoirs must not be in or pool: other pixels read those records");
  AreaDev A;
  if (int rc = risArea(c, p->flags, stream, A)) return rc;
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    ReuseDev Q{};
    fillGbuffer(Q, c, gb, out, p->minT);
    Q.gbDiffuse = gb->materialDiffuse;
    Q.gbSpecRough = gb->materialSpecRough;
    Q.in = reinterpret_cast<const uint4*>(p->in);
    Q.res = reinterpret_cast<uint4*>(p->outReservoirs);
    if (p->neighbors) {
      Q.poolGbPosition = f4(p->poolGbuffer->worldPosition);
      Q.poolGbNormal = p->poolGbuffer->worldNormal;
      Q.poolGbDiffuse = p->poolGbuffer->materialDiffuse;
      Q.poolGbSpecRough = p->poolGbuffer->materialSpecRough;
      Q.pool = reinterpret_cast<const uint4*>(p->pool);
      Q.neighborIndex = p->neighborIndex;
      Q.poolNum = c->frame.W * c->frame.H;
    }
    for (int k = 0; k < 3; k++) {
      Q.camPos[k] = ggx ? c->cam.posW[k] : 0.0f;
      Q.poolCamPos[k] = p->poolCameraPos[k];
    }
    Q.neighbors = p->neighbors;
    Q.inM = p->inM;
    Q.poolM = p->poolM;
    Q.maxM = p->maxM;
    Q.normalMin = p->normalMin;
    Q.planeMax = p->planeMax;
    Q.clampUpper = p->clampUpper;
    Q.frameCount = p->frameCount;
    Q.width = c->frame.W;
    Q.height = c->frame.H;
    Q.radius = drawn ? p->radius : 0u;
    launchReuse(c->scene.S, Q, A, true, ggx, c->rayCursor, c->grids, c->numCUs, st);
  });
}

int bdpt_motion_query(bdpt_ctx* c, const bdpt_motion_desc* d, void* stream) {
  if (!c || !d) return BDPT_E_INVALID;
  if (int rc = needScene(c, "motion_query")) return rc;
  if (!c->scene.prevPose) return refuse(c, BDPT_E_STATE, "motion_query", "no previous pose (bdpt_prepare(BDPT_PREPARE_MOTION) first)");
  if (d->reserved) return refuse(c, BDPT_E_INVALID, "motion_query", "reserved must be 0");
  if (!d->num) return BDPT_OK;
  if (!aligned(d->hits, 16) || !aligned(d->prevPositions, 16) || (d->numDevice && !aligned(d->numDevice, 4)))
    return refuse(c, BDPT_E_INVALID, "motion_query", "hits or prevPositions missing or not aligned (16 bytes; numDevice 4)");
  return enqueueQuery(c, stream, [&](hipStream_t st) {
    launchMotionQuery(c->scene.prevPose, c->scene.numTriangles, f4(d->hits), d->num, d->numDevice, f4(d->prevPositions), st);
  });
}

}  // extern "C"
