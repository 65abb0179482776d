// api_deform.cpp — moving geometry of the C ABI (include/bdpt.h): bdpt_update_geometry and bdpt_set_lights, the refit
// plan behind them, skins and morph targets (bdpt_set_skin / bdpt_set_morph, one deformation pass behind
// bdpt_update_skinned and bdpt_update_morphed, the same arithmetic on the host) and the previous pose.  The updates and
// bdpt_keep_pose enqueue on the caller's stream and can be captured once the plan exists
// (bdpt_prepare(BDPT_PREPARE_REFIT)) and their inputs are device pointers: host-pointer inputs are staged through pinned
// memory.  What allocates and synchronises the device, and so refuses a capturing stream: the ensure* functions' first
// call, bdpt_set_skin and bdpt_set_morph (transactional: a failure leaves the old one in place) and bdpt_get_refit_info.
#include <atomic>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "api_common.hpp"

using namespace bdpt;

// (the three below: declared in api_common.hpp)
// refit (refit.hip, bvh.h "refit"): the plan (a top-down pass over the records, read back once) and the refit's scratch;
// not while capturing
int bdpt::ensureRefit(bdpt_ctx* c, hipStream_t st) {
  if (c->scene.refitReady) return BDPT_OK;
  if (streamIsCapturing(st)) return refuse(c, BDPT_E_STATE, "update", "the first update needs bdpt_prepare(BDPT_PREPARE_REFIT) before stream capture");
  HIPCHK(c, hipDeviceSynchronize());
  BvhRefitPlan plan;
  {
    std::vector<BvhRec> recs(c->scene.S.numRecs);
    HIPCHK(c, hipMemcpy(recs.data(), c->scene.S.recs, recs.size() * sizeof(BvhRec), hipMemcpyDeviceToHost));
    std::string err;
    if (!bvhRefitMakePlan(recs.data(), recs.size(), plan, err)) {
      fail(c, err);
      return BDPT_E_HIP;
    }
  }
  const size_t nn = std::max<size_t>(plan.nodes.size(), 1);
  RefitDev R{};
  const BvhRefitNode* dNodes = nullptr;
  const uint32_t* dOrder = nullptr;
  int rc;
  if ((rc = devUpload(c, c->scene.allocs, &dNodes, plan.nodes.data(), plan.nodes.size())) ||
      (rc = devUpload(c, c->scene.allocs, &dOrder, plan.levelOrder.data(), plan.levelOrder.size())) ||
      (rc = devAlloc(c, c->scene.allocs, &R.box, nn * 6)) || (rc = devAlloc(c, c->scene.allocs, &R.childArea, nn * 4)) ||
      (rc = devAlloc(c, c->scene.allocs, &R.partial, (size_t)kRefitPartials * 6)) || (rc = devAlloc(c, c->scene.allocs, &R.pad, 1)))
    return rc;
  R.nodes = dNodes;
  R.levelOrder = dOrder;
  R.levelStart = plan.levelStart;
  R.numNodes = (uint32_t)plan.nodes.size();
  c->scene.refit = std::move(R);
  c->scene.refitPlan = std::move(plan);
  c->scene.refitReady = true;
  return BDPT_OK;
}

// bdpt_prepare(BDPT_PREPARE_REFIT_PIECES): the plan as above, then the regions of the tree AS BUILT (bvh.h "piece-tight
// refit", refit.hip k_refit_regions); from then on launchRefit runs its piece-tight instance
int bdpt::ensureRefitPieces(bdpt_ctx* c) {
  if (c->scene.refitReady && c->scene.refit.region) return BDPT_OK;
  if (c->scene.numUpdates) {
    fail(c, "prepare: BDPT_PREPARE_REFIT_PIECES derives the regions from the tree as built: not after an update (bdpt_set_scene first)");
    return BDPT_E_STATE;
  }
  if (streamIsCapturing(c->lastStream)) {
    fail(c, "prepare: BDPT_PREPARE_REFIT_PIECES allocates and synchronises: not inside a stream capture");
    return BDPT_E_STATE;
  }
  if (int rc = ensureRefit(c, nullptr)) return rc;
  float* region = nullptr;
  if (int rc = devAlloc(c, c->scene.allocs, &region, (size_t)c->scene.S.numRecs * kPieceFloats)) return rc;
  HIPCHK(c, hipDeviceSynchronize());
  launchRefitRegions(c->scene.refit, reinterpret_cast<const BvhRec*>(c->scene.S.recs), region, nullptr);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipDeviceSynchronize());
  c->scene.refit.region = region;
  return BDPT_OK;
}

// motion (motion.hip): the previous pose of bdpt_prepare(BDPT_PREPARE_MOTION), which bdpt_keep_pose renews
int bdpt::allocPrevPose(bdpt_ctx* c) {
  if (c->scene.prevPose) return BDPT_OK;
  if (streamIsCapturing(c->lastStream)) {
    fail(c, "prepare: BDPT_PREPARE_MOTION allocates and synchronises: not inside a stream capture");
    return BDPT_E_STATE;
  }
  float4* pose = nullptr;
  if (int rc = devAlloc(c, c->scene.allocs, &pose, (size_t)c->scene.numTriangles * 3)) return rc;
  HIPCHK(c, hipDeviceSynchronize());  // (updates in flight on any stream: the first previous pose is the current one)
  launchKeepPose(c->scene.S.shade, c->scene.numTriangles, pose, nullptr);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipDeviceSynchronize());
  c->scene.prevPose = pose;
  return BDPT_OK;
}

extern "C" {

// ---- animated scenes: refit in place (refit.hip, bvh.h "refit") ----
namespace {
// host arrays -> pinned memory (now) -> device copies (on st); arrays[k] may be null
int stageHostArrays(bdpt_ctx* c, const void* const* arrays, const size_t* bytes, int n, float** dst, hipStream_t st) {
  size_t total = 0;
  for (int k = 0; k < n; k++) total += arrays[k] ? (bytes[k] + 255) / 256 * 256 : 0;
  if (c->scene.stageInFlight) HIPCHK(c, hipEventSynchronize(c->evStage));  // the copies of the last update have read the buffer
  c->scene.stageInFlight = false;
  if (total > c->pinnedBytes) {
    if (c->pinned) HIPCHK(c, hipHostFree(c->pinned));
    c->pinned = nullptr;
    c->pinnedBytes = 0;
    if (hipHostMalloc(&c->pinned, total, hipHostMallocDefault) != hipSuccess) return refuse(c, BDPT_E_NOMEM, "update", "pinned staging memory");
    c->pinnedBytes = total;
  }
  size_t off = 0;
  for (int k = 0; k < n; k++) {
    if (!arrays[k]) continue;
    std::memcpy(static_cast<char*>(c->pinned) + off, arrays[k], bytes[k]);
    HIPCHK(c, hipMemcpyAsync(dst[k], static_cast<char*>(c->pinned) + off, bytes[k], hipMemcpyHostToDevice, st));
    off += (bytes[k] + 255) / 256 * 256;
  }
  HIPCHK(c, hipEventRecord(c->evStage, st));
  c->scene.stageInFlight = true;
  return BDPT_OK;
}
// the light cube maps of the occluder hints, re-traced on st
void retraceLightMaps(bdpt_ctx* c, hipStream_t st) {
  if (c->scene.hints && c->scene.lightMaps) launchLightMaps(c->scene.S, c->scene.lightMaps, c->scene.S.lightMapRes, st);
}

// What every update ends with, on st: the refit to the device arrays `pos` (and `nrm`), the emitter table's refresh, the
// bitangent copy, the light maps' re-trace unless kept.
int updateTail(bdpt_ctx* c, const float* pos, const float* nrm, const float* bit, uint32_t flags, hipStream_t st) {
  const size_t nv3 = (size_t)c->scene.numVertices * 3;
  const SceneDev& S = c->scene.S;
  launchRefit(c->scene.refit, reinterpret_cast<BvhRec*>(const_cast<uint4*>(S.recs)), const_cast<float4*>(S.shade), S.indices, c->scene.numTriangles, pos, nrm, st);
  if (c->scene.areaReady) launchAreaRefresh(c->scene.S, c->scene.area, c->scene.areaBlockSum, c->scene.areaBlockLast, st);  // weights and CDF of the new areas
  if (bit) HIPCHK(c, hipMemcpyAsync(const_cast<float*>(c->scene.S.bitangents), bit, nv3 * 4, hipMemcpyDeviceToDevice, st));
  if (!(flags & BDPT_UPDATE_KEEP_LIGHT_MAPS)) retraceLightMaps(c, st);
  HIPCHK(c, hipGetLastError());
  c->frame.hintCamValid = false;
  c->scene.numUpdates++;
  c->lastStream = st;
  return BDPT_OK;
}
}  // namespace

int bdpt_update_geometry(bdpt_ctx* c, const bdpt_geometry_update* u, void* stream) {
  if (!c || !u) return BDPT_E_INVALID;
  if (int rc = needScene(c, "update")) return rc;
  if (!u->positions || u->numVertices != c->scene.numVertices || u->memory > BDPT_MEMORY_DEVICE || (u->flags & ~BDPT_UPDATE_KEEP_LIGHT_MAPS)) {
    fail(c, u->numVertices != c->scene.numVertices ? "update: numVertices differs from the scene's" : "update: positions missing or bad memory / flags");
    return BDPT_E_INVALID;
  }
  if (u->bitangents && !c->scene.S.hasBitangents) return refuse(c, BDPT_E_INVALID, "update", "bitangents given for a scene that has none");
  const size_t nv3 = (size_t)c->scene.numVertices * 3;
  if (u->memory == BDPT_MEMORY_HOST) {
    std::atomic<int> bad{0};
    hostParallelFor(nv3, [&](size_t i0, size_t i1) {
      for (size_t i = i0; i < i1; i++)
        if (!bvhCoordInRange(u->positions[i])) {  // (bvh.h kBvhMaxCoord; false for a NaN)
          bad.store(1);
          return;
        }
    });
    if (bad.load()) return refuse(c, BDPT_E_INVALID, "update", "a vertex position is not finite or lies beyond 2^60");
  }
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = ensureRefit(c, st)) return rc;
  const float* pos = u->positions;
  const float* nrm = u->normals;
  const float* bit = u->bitangents;
  if (u->memory == BDPT_MEMORY_HOST) {
    const float* in[3] = {u->positions, u->normals, u->bitangents};
    for (int k = 0; k < 3; k++)
      if (in[k] && !c->scene.stage[k]) {
        if (streamIsCapturing(st)) {
          fail(c, "update: host-pointer inputs allocate their device copies on first use: not while capturing");
          return BDPT_E_STATE;
        }
        if (int rc = devAlloc(c, c->scene.allocs, &c->scene.stage[k], nv3)) return rc;
      }
    if (int rc = orderAfterLast(c, st)) return rc;
    const void* arrays[3] = {in[0], in[1], in[2]};
    const size_t bytes[3] = {nv3 * 4, nv3 * 4, nv3 * 4};
    if (int rc = stageHostArrays(c, arrays, bytes, 3, c->scene.stage, st)) return rc;
    pos = c->scene.stage[0];
    nrm = in[1] ? c->scene.stage[1] : nullptr;
    bit = in[2] ? c->scene.stage[2] : nullptr;
  } else {
    if (int rc = orderAfterLast(c, st)) return rc;
  }
  return updateTail(c, pos, nrm, bit, u->flags, st);
}

// ---- skinning and morph targets: bdpt_set_skin / bdpt_set_morph, one deformation pass behind bdpt_update_skinned and
// bdpt_update_morphed (deform.hip), and the same arithmetic on the host ----
namespace {
// the checks of a bdpt_skin_desc that need no context; `what` prefixes the message
int checkSkinDesc(bdpt_ctx* c, const bdpt_skin_desc* d, const char* what) {
  const std::string w(what);
  if (!d->positions || !d->boneWeights || !d->boneIds || d->reserved[0] || d->reserved[1] || d->numBones == 0) {
    fail(c, w + ": positions, boneWeights and boneIds are required, numBones >= 1 and reserved 0");
    return BDPT_E_INVALID;
  }
  if (d->numBones > BDPT_MAX_BONES) {
    fail(c, w + ": more than BDPT_MAX_BONES bones");
    return BDPT_E_LIMIT;
  }
  std::atomic<int> bad{0};  // 1 = position, 2 = weight, 3 = id
  hostParallelFor(d->numVertices, [&](size_t v0, size_t v1) {
    for (size_t v = v0; v < v1; v++) {
      const float* p = d->positions + v * 3;
      const float* wt = d->boneWeights + v * 4;
      if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) bad.store(1);
      if (!(std::isfinite(wt[0]) && std::isfinite(wt[1]) && std::isfinite(wt[2]) && std::isfinite(wt[3]))) {
        bad.store(2);
        continue;
      }
      if (skinIsStatic(wt)) continue;  // (its ids are neither checked nor read)
      for (int k = 0; k < 4; k++)
        if (d->boneIds[v * 4 + (size_t)k] >= d->numBones) bad.store(3);
    }
  });
  if (bad.load()) {
    fail(c, w + (bad.load() == 1 ? ": a rest position is not finite" : bad.load() == 2 ? ": a bone weight is not finite" : ": a bone id >= numBones on a vertex with a weight"));
    return BDPT_E_INVALID;
  }
  return BDPT_OK;
}

// The vertex loop of bdpt_host_skin and bdpt_host_morph: the base (with a skin, its rest pose), morphed if `m`, then
// skinned, or copied for a static vertex and without a skin.
void hostDeform(size_t numVertices, const float* baseP, const float* baseN, const float* baseB, const MorphCsr* m, const float* weights,
                const bdpt_skin_desc* skin, const float* bones, const float* normalBones, float* outP, float* outN, float* outB) {
  const float* dN = m && !m->dNrm.empty() ? m->dNrm.data() : nullptr;
  const float* dB = m && !m->dBit.empty() ? m->dBit.data() : nullptr;
  withFlag(baseN != nullptr, [&](auto hasN) {
    withFlag(baseB != nullptr, [&](auto hasB) {
      constexpr bool N = decltype(hasN)::value, B = decltype(hasB)::value;
      hostParallelFor(numVertices, [&](size_t v0, size_t v1) {
        for (size_t v = v0; v < v1; v++) {
          const size_t o = v * 3;
          float p[3], n[3] = {0.0f, 0.0f, 0.0f}, b[3] = {0.0f, 0.0f, 0.0f};
          for (int k = 0; k < 3; k++) {
            p[k] = baseP[o + k];
            if (N) n[k] = baseN[o + k];
            if (B) b[k] = baseB[o + k];
          }
          if (m) morphVertex(m->target.data(), m->dPos.data(), dN, dB, weights, m->start[v], m->start[v + 1], p, n, b);
          const float* w = skin ? skin->boneWeights + v * 4 : nullptr;
          if (skin && !skinIsStatic(w)) {
            skinVertex<N, B>(bones, normalBones, skin->boneIds + v * 4, w, p, n, b, outP + o, N ? outN + o : nullptr, B ? outB + o : nullptr);
            continue;
          }
          for (int k = 0; k < 3; k++) {
            outP[o + k] = p[k];
            if (N) outN[o + k] = n[k];
            if (B) outB[o + k] = b[k];
          }
        }
      });
    });
  });
}

// the context's deformed streams: the skin's with a skin, the morph's without
struct DeformOut {
  float *pos, *nrm, *bit;
};
DeformOut deformOut(const bdpt_ctx* c) {
  const SkinDev& K = c->scene.skin.dev;
  const MorphDev& M = c->scene.skin.morph.dev;
  return c->scene.skin.have ? DeformOut{K.pos, K.nrm, K.bit} : DeformOut{M.pos, M.nrm, M.bit};
}
int deformedBuffers(const bdpt_ctx* c, const float** positions, const float** normals, const float** bitangents) {
  const DeformOut o = deformOut(c);
  *positions = o.pos;
  *normals = o.nrm;
  *bitangents = o.bit;
  return BDPT_OK;
}

// What bdpt_update_skinned (weights null) and bdpt_update_morphed do with arguments that passed their checks: the
// finiteness scan of host inputs, their staging, the deformation pass and the refit.  `what` prefixes the messages.
int updateDeformed(bdpt_ctx* c, const char* what, const float* weights, const float* bones, const float* nbones, uint32_t memory, uint32_t flags,
                   void* stream) {
  const std::string w(what);
  const MorphDev* M = weights ? &c->scene.skin.morph.dev : nullptr;
  const SkinDev* K = c->scene.skin.have ? &c->scene.skin.dev : nullptr;
  const size_t nw = M ? M->numTargets : 0, pal = K ? (size_t)K->numBones * 16 : 0;
  const bool host = memory == BDPT_MEMORY_HOST;
  if (host) {
    bool finite = true;
    for (size_t t = 0; t < nw; t++) finite = finite && std::isfinite(weights[t]);
    for (size_t i = 0; i < pal; i++) finite = finite && std::isfinite(bones[i]) && (!nbones || std::isfinite(nbones[i]));
    if (!finite) {
      fail(c, w + (M ? ": a weight or a bone matrix element is not finite" : ": a bone matrix element is not finite"));
      return BDPT_E_INVALID;
    }
  }
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = ensureRefit(c, st)) return rc;  // (bdpt_set_skin / bdpt_set_morph made the plan: nothing to do)
  if (host && streamIsCapturing(st)) {
    fail(c, w + ": host-pointer " + (M ? "weights and palettes" : "palettes") + " are staged through pinned memory: not while capturing");
    return BDPT_E_STATE;
  }
  if (int rc = orderAfterLast(c, st)) return rc;
  if (host) {
    const void* arrays[3] = {weights, bones, nbones};
    const size_t bytes[3] = {nw * 4, pal * 4, pal * 4};
    float* dst[3] = {c->scene.skin.morph.weights, c->scene.skin.palette[0], c->scene.skin.palette[1]};
    if (int rc = stageHostArrays(c, arrays, bytes, 3, dst, st)) return rc;
    if (weights) weights = dst[0];
    if (bones) bones = dst[1];
    if (nbones) nbones = dst[2];
  }
  launchDeform(M, weights, K, bones, nbones, kSkinPathAuto, st);
  const DeformOut o = deformOut(c);
  return updateTail(c, o.pos, o.nrm, o.bit, flags, st);
}

}  // namespace

int bdpt_host_skin(const bdpt_skin_desc* d, const float* bones, const float* normalBones, float* outPositions, float* outNormals,
                   float* outBitangents) {
  if (!d || !bones || !outPositions) return BDPT_E_INVALID;
  if ((d->normals && (!normalBones || !outNormals)) || (d->bitangents && !outBitangents)) return BDPT_E_INVALID;
  if (int rc = checkSkinDesc(nullptr, d, "host_skin")) return rc;
  hostDeform(d->numVertices, d->positions, d->normals, d->bitangents, nullptr, nullptr, d, bones, normalBones, outPositions, outNormals, outBitangents);
  return BDPT_OK;
}

int bdpt_set_skin(bdpt_ctx* c, const bdpt_skin_desc* d) {
  if (!c) return BDPT_E_INVALID;
  if (int rc = needScene(c, "set_skin")) return rc;
  if (d) {
    if (d->numVertices != c->scene.numVertices) return refuse(c, BDPT_E_INVALID, "set_skin", "numVertices differs from the scene's");
    if (d->bitangents && !c->scene.S.hasBitangents) return refuse(c, BDPT_E_INVALID, "set_skin", "bitangents given for a scene that has none");
    if (int rc = checkSkinDesc(c, d, "set_skin")) return rc;
  }
  ENTER(c);
  if (streamIsCapturing(c->lastStream)) return refuse(c, BDPT_E_STATE, "set_skin", "not inside a stream capture (it allocates and synchronises)");
  if (d)
    if (int rc = ensureRefit(c, c->lastStream)) return rc;  // (before the old skin goes: a failure leaves it in place)
  HIPCHK(c, hipDeviceSynchronize());
  SkinState next;  // built here, committed at the end: a failure leaves the old skin in place
  DevPool& pool = next.allocs;
  SkinDev& K = next.dev;
  float** palette = next.palette;
  if (d) {
    const size_t nv = d->numVertices, nv3 = nv * 3, pal = (size_t)d->numBones * 16;
    int rc;
    if ((rc = devUpload(c, pool, &K.restPos, d->positions, nv3)) || (d->normals && (rc = devUpload(c, pool, &K.restNrm, d->normals, nv3))) ||
        (d->bitangents && (rc = devUpload(c, pool, &K.restBit, d->bitangents, nv3))) || (rc = devUpload(c, pool, &K.weights, d->boneWeights, nv * 4)) ||
        (rc = devUpload(c, pool, &K.ids, d->boneIds, nv * 4)) || (rc = devAlloc(c, pool, &K.pos, nv3)) ||
        (d->normals && (rc = devAlloc(c, pool, &K.nrm, nv3))) || (d->bitangents && (rc = devAlloc(c, pool, &K.bit, nv3))) ||
        (rc = devAlloc(c, pool, &palette[0], pal)) || (d->normals && (rc = devAlloc(c, pool, &palette[1], pal))))
      return rc;
    // until the first update the skinned streams hold the rest pose, the palettes zeros
    hipError_t e = hipMemcpy(K.pos, K.restPos, nv3 * 4, hipMemcpyDeviceToDevice);
    if (e == hipSuccess && K.nrm) e = hipMemcpy(K.nrm, K.restNrm, nv3 * 4, hipMemcpyDeviceToDevice);
    if (e == hipSuccess && K.bit) e = hipMemcpy(K.bit, K.restBit, nv3 * 4, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipMemset(palette[0], 0, pal * 4);
    if (e == hipSuccess && palette[1]) e = hipMemset(palette[1], 0, pal * 4);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
      fail(c, std::string("set_skin: ") + hipGetErrorString(e));
      return BDPT_E_HIP;
    }
    K.numVertices = d->numVertices;
    K.numBones = d->numBones;
  }
  next.have = d != nullptr;
  dropSkin(c->scene.skin);  // (and the morph: its base and its outputs were this skin's, or it had none)
  c->scene.skin = std::move(next);
  return BDPT_OK;
}

int bdpt_update_skinned(bdpt_ctx* c, const bdpt_skin_update* u, void* stream) {
  if (!c || !u) return BDPT_E_INVALID;
  if (int rc = needScene(c, "update_skinned")) return rc;
  if (!c->scene.skin.have) return refuse(c, BDPT_E_STATE, "update_skinned", "no skin (bdpt_set_skin first)");
  const SkinDev& K = c->scene.skin.dev;
  if (!u->bones || (K.nrm && !u->normalBones) || u->numBones != K.numBones || u->memory > BDPT_MEMORY_DEVICE ||
      (u->flags & ~BDPT_UPDATE_KEEP_LIGHT_MAPS) || u->reserved) {
    fail(c, u->numBones != K.numBones ? "update_skinned: numBones differs from the skin's"
                                      : "update_skinned: bones (or normalBones, for a skin with normals) missing, or bad memory / flags / reserved");
    return BDPT_E_INVALID;
  }
  return updateDeformed(c, "update_skinned", nullptr, u->bones, K.nrm ? u->normalBones : nullptr, u->memory, u->flags, stream);
}

int bdpt_skinned_buffers(bdpt_ctx* c, const float** positions, const float** normals, const float** bitangents) {
  if (!c || !positions || !normals || !bitangents) return BDPT_E_INVALID;
  if (!c->scene.have || !c->scene.skin.have) return refuse(c, BDPT_E_STATE, "skinned_buffers", "no skin (bdpt_set_skin first)");
  return deformedBuffers(c, positions, normals, bitangents);
}

namespace {
// The checks of a bdpt_morph_desc.  haveSkin: the base is a skin's rest pose, which has normals / bitangents where
// skinN / skinB; `what` prefixes the message.
int checkMorphDesc(bdpt_ctx* c, const bdpt_morph_desc* d, bool haveSkin, bool skinN, bool skinB, const char* what) {
  const std::string w(what);
  if (!d->targetStart || !d->vertex || !d->dPositions || d->reserved[0] || d->reserved[1] || d->numTargets == 0) {
    fail(c, w + ": targetStart, vertex and dPositions are required, numTargets >= 1 and reserved 0");
    return BDPT_E_INVALID;
  }
  if (d->numTargets > BDPT_MAX_MORPH_TARGETS) {
    fail(c, w + ": more than BDPT_MAX_MORPH_TARGETS targets");
    return BDPT_E_LIMIT;
  }
  if (haveSkin) {
    if (d->positions || d->normals || d->bitangents) {
      fail(c, w + ": the base is the skin's rest pose: positions, normals and bitangents must be NULL");
      return BDPT_E_INVALID;
    }
  } else if (!d->positions) {
    fail(c, w + ": positions (the base pose) are required without a skin");
    return BDPT_E_INVALID;
  }
  if ((d->dNormals && !(haveSkin ? skinN : d->normals != nullptr)) || (d->dBitangents && !(haveSkin ? skinB : d->bitangents != nullptr))) {
    fail(c, w + ": deltas for a stream the base lacks");
    return BDPT_E_INVALID;
  }
  if (d->targetStart[0] != 0) {
    fail(c, w + ": targetStart[0] is not 0");
    return BDPT_E_INVALID;
  }
  for (uint32_t t = 0; t < d->numTargets; t++)
    if (d->targetStart[t + 1] < d->targetStart[t]) {
      fail(c, w + ": targetStart decreases");
      return BDPT_E_INVALID;
    }
  const size_t ne = d->targetStart[d->numTargets];
  if (ne >= ((size_t)1 << 31)) {
    fail(c, w + ": 2^31 entries or more");
    return BDPT_E_LIMIT;
  }
  for (uint32_t t = 0; t < d->numTargets; t++)
    for (size_t e = d->targetStart[t]; e < d->targetStart[t + 1]; e++)
      if (d->vertex[e] >= d->numVertices || (e > d->targetStart[t] && d->vertex[e] <= d->vertex[e - 1])) {
        fail(c, w + ": a vertex id >= numVertices, or ids not strictly ascending within a target");
        return BDPT_E_INVALID;
      }
  std::atomic<int> bad{0};
  const float* deltas[3] = {d->dPositions, d->dNormals, d->dBitangents};
  const float* base[3] = {d->positions, d->normals, d->bitangents};
  for (int k = 0; k < 3; k++) {
    if (deltas[k])
      hostParallelFor(ne * 3, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++)
          if (!std::isfinite(deltas[k][i])) bad.store(1);
      });
    if (base[k])
      hostParallelFor((size_t)d->numVertices * 3, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++)
          if (!std::isfinite(base[k][i])) bad.store(2);
      });
  }
  if (bad.load()) {
    fail(c, w + (bad.load() == 1 ? ": a delta is not finite" : ": a base value is not finite"));
    return BDPT_E_INVALID;
  }
  return BDPT_OK;
}
}  // namespace

int bdpt_host_morph(const bdpt_morph_desc* d, const bdpt_skin_desc* skin, const float* weights, const float* bones, const float* normalBones,
                    float* outPositions, float* outNormals, float* outBitangents) {
  if (!d || !weights || !outPositions) return BDPT_E_INVALID;
  if (skin) {
    if (skin->numVertices != d->numVertices || !bones || (skin->normals && !normalBones)) return BDPT_E_INVALID;
    if (int rc = checkSkinDesc(nullptr, skin, "host_morph")) return rc;
  } else if (bones || normalBones) {
    return BDPT_E_INVALID;
  }
  if (int rc = checkMorphDesc(nullptr, d, skin != nullptr, skin && skin->normals, skin && skin->bitangents, "host_morph")) return rc;
  const float* baseP = skin ? skin->positions : d->positions;
  const float* baseN = skin ? skin->normals : d->normals;
  const float* baseB = skin ? skin->bitangents : d->bitangents;
  if ((baseN && !outNormals) || (baseB && !outBitangents)) return BDPT_E_INVALID;
  for (uint32_t t = 0; t < d->numTargets; t++)
    if (!std::isfinite(weights[t])) return BDPT_E_INVALID;
  const MorphCsr m = morphBuildCsr(d->numVertices, d->numTargets, d->targetStart, d->vertex, d->dPositions, d->dNormals, d->dBitangents);
  hostDeform(d->numVertices, baseP, baseN, baseB, &m, weights, skin, bones, normalBones, outPositions, outNormals, outBitangents);
  return BDPT_OK;
}

int bdpt_set_morph(bdpt_ctx* c, const bdpt_morph_desc* d) {
  if (!c) return BDPT_E_INVALID;
  if (int rc = needScene(c, "set_morph")) return rc;
  if (d) {
    if (d->numVertices != c->scene.numVertices) return refuse(c, BDPT_E_INVALID, "set_morph", "numVertices differs from the scene's");
    if ((d->bitangents || d->dBitangents) && !c->scene.S.hasBitangents) {
      fail(c, "set_morph: bitangents given for a scene that has none");
      return BDPT_E_INVALID;
    }
    if (int rc = checkMorphDesc(c, d, c->scene.skin.have, c->scene.skin.dev.nrm != nullptr, c->scene.skin.dev.bit != nullptr, "set_morph")) return rc;
  }
  ENTER(c);
  if (streamIsCapturing(c->lastStream)) return refuse(c, BDPT_E_STATE, "set_morph", "not inside a stream capture (it allocates and synchronises)");
  if (d)
    if (int rc = ensureRefit(c, c->lastStream)) return rc;  // (before the old morph goes: a failure leaves it in place)
  HIPCHK(c, hipDeviceSynchronize());
  MorphState next;  // built here, committed at the end: a failure leaves the old morph in place
  DevPool& pool = next.allocs;
  MorphDev& M = next.dev;
  float*& weights = next.weights;
  if (d) {
    const MorphCsr m = morphBuildCsr(d->numVertices, d->numTargets, d->targetStart, d->vertex, d->dPositions, d->dNormals, d->dBitangents);
    const size_t nv3 = (size_t)d->numVertices * 3;
    int rc;
    if ((rc = devUpload(c, pool, &M.start, m.start.data(), m.start.size())) || (rc = devUpload(c, pool, &M.target, m.target.data(), m.target.size())) ||
        (rc = devUpload(c, pool, &M.dPos, m.dPos.data(), m.dPos.size())) ||
        (d->dNormals && (rc = devUpload(c, pool, &M.dNrm, m.dNrm.data(), m.dNrm.size()))) ||
        (d->dBitangents && (rc = devUpload(c, pool, &M.dBit, m.dBit.data(), m.dBit.size()))) ||
        (rc = devUpload(c, pool, &M.active, m.active.data(), m.active.size())) || (rc = devAlloc(c, pool, &weights, d->numTargets)) ||
        (d->positions && ((rc = devUpload(c, pool, &M.basePos, d->positions, nv3)) || (rc = devAlloc(c, pool, &M.pos, nv3)))) ||
        (d->normals && ((rc = devUpload(c, pool, &M.baseNrm, d->normals, nv3)) || (rc = devAlloc(c, pool, &M.nrm, nv3)))) ||
        (d->bitangents && ((rc = devUpload(c, pool, &M.baseBit, d->bitangents, nv3)) || (rc = devAlloc(c, pool, &M.bit, nv3)))))
      return rc;
    // until the first update the morphed streams hold the base, the weights zeros
    hipError_t e = hipMemset(weights, 0, (size_t)d->numTargets * 4);
    if (e == hipSuccess && M.pos) e = hipMemcpy(M.pos, M.basePos, nv3 * 4, hipMemcpyDeviceToDevice);
    if (e == hipSuccess && M.nrm) e = hipMemcpy(M.nrm, M.baseNrm, nv3 * 4, hipMemcpyDeviceToDevice);
    if (e == hipSuccess && M.bit) e = hipMemcpy(M.bit, M.baseBit, nv3 * 4, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
      fail(c, std::string("set_morph: ") + hipGetErrorString(e));
      return BDPT_E_HIP;
    }
    M.numVertices = d->numVertices;
    M.numTargets = d->numTargets;
    M.numActive = (uint32_t)m.active.size();
  }
  next.have = d != nullptr;
  dropMorph(c->scene.skin.morph);
  c->scene.skin.morph = std::move(next);
  return BDPT_OK;
}

int bdpt_update_morphed(bdpt_ctx* c, const bdpt_morph_update* u, void* stream) {
  if (!c || !u) return BDPT_E_INVALID;
  if (int rc = needScene(c, "update_morphed")) return rc;
  if (!c->scene.skin.morph.have) return refuse(c, BDPT_E_STATE, "update_morphed", "no morph (bdpt_set_morph first)");
  const MorphDev& M = c->scene.skin.morph.dev;
  const SkinDev* K = c->scene.skin.have ? &c->scene.skin.dev : nullptr;
  const bool needN = K && K->nrm;
  if (!u->weights || u->numTargets != M.numTargets || u->numBones != (K ? K->numBones : 0u) || (u->bones != nullptr) != (K != nullptr) ||
      (u->normalBones != nullptr) != needN || u->memory > BDPT_MEMORY_DEVICE || (u->flags & ~BDPT_UPDATE_KEEP_LIGHT_MAPS) || u->reserved[0] ||
      u->reserved[1]) {
    fail(c, u->numTargets != M.numTargets ? "update_morphed: numTargets differs from the morph's"
            : u->numBones != (K ? K->numBones : 0u)
                ? "update_morphed: numBones differs from the skin's (0 without a skin)"
                : "update_morphed: weights missing, palettes missing with a skin or given without one, or bad memory / flags / reserved");
    return BDPT_E_INVALID;
  }
  return updateDeformed(c, "update_morphed", u->weights, u->bones, u->normalBones, u->memory, u->flags, stream);
}

int bdpt_morphed_buffers(bdpt_ctx* c, const float** positions, const float** normals, const float** bitangents) {
  if (!c || !positions || !normals || !bitangents) return BDPT_E_INVALID;
  if (!c->scene.have || !c->scene.skin.morph.have) return refuse(c, BDPT_E_STATE, "morphed_buffers", "no morph (bdpt_set_morph first)");
  return deformedBuffers(c, positions, normals, bitangents);
}

int bdpt_set_lights(bdpt_ctx* c, const bdpt_light* lights, uint32_t numLights, void* stream) {
  if (!c || !lights) return BDPT_E_INVALID;
  if (int rc = needScene(c, "set_lights")) return rc;
  if (numLights > BDPT_MAX_LIGHTS) return refuse(c, BDPT_E_LIMIT, "set_lights", "more than BDPT_MAX_LIGHTS lights");
  if (numLights != c->scene.S.numLights) return refuse(c, BDPT_E_INVALID, "set_lights", "the light count differs from the scene's");
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = orderAfterLast(c, st)) return rc;
  const void* arrays[1] = {lights};
  const size_t bytes[1] = {sizeof(bdpt_light) * numLights};
  float* dst[1] = {reinterpret_cast<float*>(const_cast<SceneConst*>(c->scene.S.sc)->lights)};
  if (int rc = stageHostArrays(c, arrays, bytes, 1, dst, st)) return rc;
  retraceLightMaps(c, st);
  HIPCHK(c, hipGetLastError());
  c->frame.hintCamValid = false;
  c->lastStream = st;
  return BDPT_OK;
}

int bdpt_get_refit_info(bdpt_ctx* c, bdpt_refit_info* out) {
  if (!c || !out) return BDPT_E_INVALID;
  if (!c->scene.have) return BDPT_E_STATE;
  ENTER(c);
  *out = bdpt_refit_info{};
  out->sahCostBuilt = c->scene.bvhInfo.sahCost;
  out->sahCost = c->scene.bvhInfo.sahCost;
  out->numUpdates = c->scene.numUpdates;
  if (c->scene.numUpdates == 0) return BDPT_OK;
  HIPCHK(c, hipDeviceSynchronize());
  std::vector<float> area((size_t)c->scene.refit.numNodes * 4);
  float root[6] = {0, 0, 0, 0, 0, 0};
  if (c->scene.refit.numNodes) {
    HIPCHK(c, hipMemcpy(area.data(), c->scene.refit.childArea, area.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(root, c->scene.refit.box, sizeof(root), hipMemcpyDeviceToHost));
  }
  out->sahCost = bvhRefitSah(c->scene.refitPlan, root, area.data());
  return BDPT_OK;
}

int bdpt_keep_pose(bdpt_ctx* c, void* stream) {
  if (!c) return BDPT_E_INVALID;
  if (int rc = needScene(c, "keep_pose")) return rc;
  if (!c->scene.prevPose) return refuse(c, BDPT_E_STATE, "keep_pose", "no previous pose (bdpt_prepare(BDPT_PREPARE_MOTION) first)");
  ENTER(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = orderAfterLast(c, st)) return rc;
  launchKeepPose(c->scene.S.shade, c->scene.numTriangles, c->scene.prevPose, st);
  HIPCHK(c, hipGetLastError());
  c->lastStream = st;
  return BDPT_OK;
}

}  // extern "C"
