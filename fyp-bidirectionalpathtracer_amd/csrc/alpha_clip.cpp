// alpha_clip.cpp — see alpha_clip.h.
#include "alpha_clip.h"
#include "texture_planes.h"

#include <algorithm>
#include <cmath>

namespace bdpt {
namespace {

inline int wrapHost(int i, int n) {
  const int m = i % n;
  return (m < 0) ? m + n : m;
}

}  // namespace

// Texels the sample of cell (i, j) blends: (i, j), (i+1, j), (i, j+1), (i+1, j+1), wrapped (device_scene.hpp
// alphaTestFails).  The blend is a convex combination evaluated in fp32: it stays within [min, max] of the four up
// to a few ulps, so a cell whose largest texel is below threshold - 1e-5 always fails and one whose smallest is at or
// above threshold + 1e-5 always passes.
AlphaClipper::AlphaClipper(const bdpt_scene_desc* d) : d_(d) {
  matMask_.assign(d->numMaterials, -1);
  matVerdict_.assign(d->numMaterials, 0);
  for (uint32_t mi = 0; mi < d->numMaterials; mi++) {
    const bdpt_material& m = d->materials[mi];
    if (BDPT_FLAG_ALPHA_MODE(m.flags) == BDPT_ALPHA_MODE_OPAQUE) continue;
    const uint32_t type = BDPT_FLAG_DIFFUSE_TYPE(m.flags);
    if (type == BDPT_CHANNEL_UNUSED) {
      matVerdict_[mi] = (0.0f < m.alphaThreshold) ? 2 : 1;
    } else if (type == BDPT_CHANNEL_CONST || m.texBaseColor < 0) {
      matVerdict_[mi] = (m.baseColor[3] < m.alphaThreshold) ? 2 : 1;
    } else if ((uint32_t)m.texBaseColor < d->numTextures && d->textures[m.texBaseColor].rgba8 && d->textures[m.texBaseColor].width &&
               d->textures[m.texBaseColor].height && d->textures[m.texBaseColor].width <= 16384 && d->textures[m.texBaseColor].height <= 16384) {
      const bdpt_texture& t = d->textures[m.texBaseColor];
      Mask mk;
      mk.w = (int)t.width;
      mk.h = (int)t.height;
      const size_t W1 = (size_t)mk.w + 1;
      mk.mayPass.assign(W1 * ((size_t)mk.h + 1), 0u);
      mk.mayFail.assign(W1 * ((size_t)mk.h + 1), 0u);
      const float thr = m.alphaThreshold;
      for (int j = 0; j < mk.h; j++) {
        const int j1 = wrapHost(j + 1, mk.h);
        for (int i = 0; i < mk.w; i++) {
          const int i1 = wrapHost(i + 1, mk.w);
          const float a00 = (float)t.rgba8[((size_t)j * mk.w + i) * 4 + 3] / 255.0f, a10 = (float)t.rgba8[((size_t)j * mk.w + i1) * 4 + 3] / 255.0f;
          const float a01 = (float)t.rgba8[((size_t)j1 * mk.w + i) * 4 + 3] / 255.0f, a11 = (float)t.rgba8[((size_t)j1 * mk.w + i1) * 4 + 3] / 255.0f;
          const float hi = std::max(std::max(a00, a10), std::max(a01, a11)), lo = std::min(std::min(a00, a10), std::min(a01, a11));
          const uint32_t pass = !(hi < thr - 1e-5f) ? 1u : 0u, fail = (lo < thr + 1e-5f) ? 1u : 0u;
          const size_t o = ((size_t)j + 1) * W1 + (size_t)i + 1;
          mk.mayPass[o] = pass + mk.mayPass[o - 1] + mk.mayPass[o - W1] - mk.mayPass[o - W1 - 1];
          mk.mayFail[o] = fail + mk.mayFail[o - 1] + mk.mayFail[o - W1] - mk.mayFail[o - W1 - 1];
        }
      }
      matMask_[mi] = (int32_t)masks_.size();
      masks_.push_back(std::move(mk));
    }
  }
  for (const Mask& mk : masks_) passMasks_.push_back(BvhClipMask{mk.w, mk.h, mk.mayPass.data()});
}

// The decisions themselves are bvh_refs.h (the device builder runs the same text on copies of these tables).
BvhClipView AlphaClipper::view() const {
  return BvhClipView{d_->triMaterial, d_->indices, d_->texcoords, matMask_.data(), matVerdict_.data(), passMasks_.data()};
}

int AlphaClipper::classify(uint32_t tri) const {
  const uint32_t mat = d_->triMaterial[tri];
  if (matMask_[mat] < 0) return matVerdict_[mat];
  const double whole[3][2] = {{0.0, 0.0}, {1.0, 0.0}, {0.0, 1.0}};
  const BvhClipMask& m = passMasks_[(size_t)matMask_[mat]];
  BvhCellRect R;
  if (!bvhClipCellRect(view(), m, tri, whole, 3, R)) return 0;
  if (bvhClipCount(masks_[(size_t)matMask_[mat]].mayFail.data(), m.w, m.h, R.x0, R.x1, R.y0, R.y1) == 0) return 1;
  if (bvhClipCount(m.sat, m.w, m.h, R.x0, R.x1, R.y0, R.y1) == 0) return 2;
  return 0;
}

bool AlphaClipper::clip(uint32_t tri, double (*poly)[2], int& n) const { return bvhClipPoly(view(), tri, poly, n); }

bool AlphaClipper::tables(BvhClipTables& out) const {
  out.triMaterial = d_->triMaterial;
  out.indices = d_->indices;
  out.texcoords = d_->texcoords;
  out.numTriangles = d_->numTriangles;
  out.numVertices = d_->numVertices;
  out.matMask = matMask_;
  out.matVerdict = matVerdict_;
  out.masks.clear();
  for (const BvhClipMask& m : passMasks_) out.masks.push_back(BvhClipTables::Mask{m.w, m.h, m.sat});
  return true;
}

bool AlphaClipper::testFails(uint32_t tri, float bu, float bv) const {
  const bdpt_material& mm = d_->materials[d_->triMaterial[tri]];
  const uint32_t type = BDPT_FLAG_DIFFUSE_TYPE(mm.flags);
  float alpha = 0.0f;
  if (type == BDPT_CHANNEL_UNUSED) {
    alpha = 0.0f;
  } else if (type == BDPT_CHANNEL_CONST || mm.texBaseColor < 0) {
    alpha = mm.baseColor[3];
  } else {
    const bdpt_texture& t = d_->textures[mm.texBaseColor];
    float uvs[3][2];
    for (int k = 0; k < 3; k++) {
      const uint32_t vi = d_->indices[(size_t)tri * 3 + (size_t)k];
      uvs[k][0] = d_->texcoords ? d_->texcoords[(size_t)vi * 3] : 0.0f;
      uvs[k][1] = d_->texcoords ? d_->texcoords[(size_t)vi * 3 + 1] : 0.0f;
    }
    float u = 0, v = 0;
    const float b0 = 1.0f - bu - bv;
    u += uvs[0][0] * b0;
    v += uvs[0][1] * b0;
    u += uvs[1][0] * bu;
    v += uvs[1][1] * bu;
    u += uvs[2][0] * bv;
    v += uvs[2][1] * bv;
    const int tw = (int)t.width, th = (int)t.height;
    const float x = u * (float)tw - 0.5f, y = v * (float)th - 0.5f;
    const float x0 = std::floor(x), y0 = std::floor(y);
    const float fx = x - x0, fy = y - y0;
    const int ix0 = wrapHost(texelFloorInt(x0), tw), iy0 = wrapHost(texelFloorInt(y0), th);
    const int ix1 = wrapHost(ix0 + 1, tw), iy1 = wrapHost(iy0 + 1, th);
    const uint8_t* px = t.rgba8;
    const float t00 = (float)px[((size_t)iy0 * tw + (size_t)ix0) * 4 + 3] / 255.0f, t10 = (float)px[((size_t)iy0 * tw + (size_t)ix1) * 4 + 3] / 255.0f;
    const float t01 = (float)px[((size_t)iy1 * tw + (size_t)ix0) * 4 + 3] / 255.0f, t11 = (float)px[((size_t)iy1 * tw + (size_t)ix1) * 4 + 3] / 255.0f;
    const float top = t00 + (t10 - t00) * fx, bot = t01 + (t11 - t01) * fx;
    alpha = top + (bot - top) * fy;
  }
  return alpha < mm.alphaThreshold;
}

}  // namespace bdpt
