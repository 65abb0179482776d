// Stand-alone host program for tests/test_edge_poses_cpu.py, built with -fsanitize=undefined,float-cast-overflow: the
// functions of csrc/bvh.h that the refit kernels run (bvhQuantiseNode, bvhRefitNodeT with and without pieces,
// bvhPieceBox, bvhPadOf, bvhTriGeom) on the boxes and positions an overflowing skin produces — infinities, NaNs, the
// largest finite values, subnormals.  Nothing here may be undefined in C++: the device runs the same text, and the two
// have to agree on every input.  Also states what the conversions give: a NaN plane quantises to 0, +inf to 255.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "bvh.h"

using namespace bdpt;

static uint32_t gSum = 2166136261u;
static void mix(const void* p, size_t n) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n; i++) gSum = (gSum ^ b[i]) * 16777619u;
}

int main() {
  const float vals[] = {0.0f, -0.0f, 1.0f, -1.0f, 0.5f, 255.5f, 1e30f, -1e30f, 3.4e38f, -3.4e38f, INFINITY, -INFINITY, NAN, 1e-40f, -1e-40f, 1e19f};
  const int nv = (int)(sizeof(vals) / sizeof(vals[0]));
  int failures = 0;

  // 1. one node's quantisation: child 0 takes every (lo, hi) pair on every axis, child 1 is the unit box
  for (int i = 0; i < nv; i++)
    for (int j = 0; j < nv; j++)
      for (int nk = 1; nk <= 4; nk++) {
        float clo[4][3], chi[4][3];
        for (int k = 0; k < 4; k++)
          for (int a = 0; a < 3; a++) {
            clo[k][a] = k == 0 ? vals[i] : 0.0f;
            chi[k][a] = k == 0 ? vals[j] : 1.0f;
          }
        uint32_t w[10];
        bvhQuantiseNode(clo, chi, nk, w);
        mix(w, sizeof(w));
        if (nk == 2 && std::isnan(vals[i]) && std::isnan(vals[j]) && ((w[4] & 0xffu) != 0u || (w[7] & 0xffu) != 0u)) {
          std::printf("a NaN box must quantise to the planes 0 / 0, got %u / %u\n", w[4] & 0xffu, w[7] & 0xffu);
          failures++;
        }
        if (nk == 2 && vals[i] == 0.0f && std::isinf(vals[j]) && vals[j] > 0 && (w[7] & 0xffu) != 255u) {
          std::printf("a box up to +inf must quantise its upper plane to 255, got %u\n", w[7] & 0xffu);
          failures++;
        }
      }

  // 2. one node of a refit with two leaf children (one and two references), plainly and by pieces, every value in turn
  //    as a coordinate of every vertex, and as the pad
  BvhRec recs[4 + kBvhPadRecs];
  std::memset(recs, 0, sizeof(recs));
  recs[0].w[3] = 3u << 24;  // both children are leaves
  recs[0].w[10] = 1;        // childBase
  recs[0].w[11] = 1u << 8;  // child 1 starts one record behind child 0
  for (uint32_t t = 0; t < 3; t++) recs[1 + t].w[3] = t;  // prim
  BvhRefitNode nd;
  nd.rec = 0;
  nd.nk = 2;
  nd.kid[0] = kRefitLeaf | 1u;
  nd.kid[1] = kRefitLeaf | 2u;
  nd.kid[2] = nd.kid[3] = 0;
  const uint32_t idx[9] = {0, 1, 2, 3, 4, 5, 6, 7, 8};
  float region[4 * kPieceFloats];
  const float whole[kPieceFloats] = {0, 1, 0, 1, 0, 1}, part[kPieceFloats] = {0.25f, 0.75f, 0.0f, 0.5f, 0.25f, 1.0f};
  std::memcpy(region + kPieceFloats, whole, sizeof(whole));
  std::memcpy(region + 2 * kPieceFloats, part, sizeof(part));
  std::memcpy(region + 3 * kPieceFloats, part, sizeof(part));
  for (int i = 0; i < nv; i++)
    for (int slot = 0; slot < 27; slot++)
      for (int j = 0; j < nv; j += 5) {
        float pos[27];
        for (int k = 0; k < 27; k++) pos[k] = (float)((k * 7) % 5) - 2.0f + 0.25f * (float)(k % 3);
        pos[slot] = vals[i];
        pos[(slot + 4) % 27] = vals[j];
        float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
        for (int t = 0; t < 3; t++) {
          float v0[3], e1[3], e2[3], tl[3], th[3];
          bvhTriGeom(pos + 9 * t, pos + 9 * t + 3, pos + 9 * t + 6, v0, e1, e2, tl, th);
          for (int a = 0; a < 3; a++) {
            lo[a] = tl[a] < lo[a] ? tl[a] : lo[a];
            hi[a] = hi[a] < th[a] ? th[a] : hi[a];
          }
        }
        const float pads[2] = {bvhPadOf(lo, hi, true), vals[i]};
        for (float pad : pads) {
          float box[6], area[4];
          bvhRefitNode(nd, 0, recs, pos, idx, box, area, pad);
          mix(recs, 4 * sizeof(BvhRec));
          bvhRefitNodePieces(nd, 0, recs, pos, idx, box, area, pad, region);
          mix(recs, 4 * sizeof(BvhRec));
          mix(area, sizeof(area));
        }
      }

  // 3. a piece box from regions at and beyond their edges
  for (int i = 0; i < nv; i++)
    for (int j = 0; j < nv; j++) {
      const float v0[3] = {vals[i], 1.0f, -2.0f}, e1[3] = {1.0f, vals[j], 0.5f}, e2[3] = {-0.5f, 2.0f, vals[i]};
      const float g[kPieceFloats] = {0.0f, vals[j] > 1.0f ? 1.0f : (vals[j] > 0.0f ? vals[j] : 0.0f), 0.25f, 1.0f, 0.0f, 1.0f};
      float lo[3] = {-1e30f, -1e30f, -1e30f}, hi[3] = {1e30f, 1e30f, 1e30f};
      bvhPieceBox(v0, e1, e2, g, lo, hi);
      mix(lo, sizeof(lo));
      mix(hi, sizeof(hi));
    }

  // 4. a piece box never leaves its triangle's five-point box: far from the origin the corners (v0 + u e1) + v e2 round at
  //    the size of the coordinates and do step outside it (counted: the family reaches its edge), the intersection with
  //    the box bvhPieceBox is handed brings them back
  {
    uint32_t rnd = 12345u, outside = 0;
    auto next = [&rnd] {
      rnd = rnd * 1664525u + 1013904223u;
      return (float)(rnd >> 8) / 16777216.0f;
    };
    const float regions[3][kPieceFloats] = {{0.0f, 1.0f, 0.0f, 1.0f, 0.5f, 1.0f}, {0.25f, 1.0f, 0.0f, 0.75f, 0.0f, 1.0f}, {0.0f, 0.5f, 0.5f, 1.0f, 0.75f, 1.0f}};
    for (int i = 0; i < 30000; i++) {
      float a[3], b[3], c[3], v0[3], e1[3], e2[3], tl[3], th[3];
      for (int k = 0; k < 3; k++) {
        const float base = 1.0e6f * (float)(k + 1);
        a[k] = base + 20.0f * next();
        b[k] = base + 20.0f * next();
        c[k] = base + 20.0f * next();
      }
      bvhTriGeom(a, b, c, v0, e1, e2, tl, th);
      const float* g = regions[i % 3];
      for (int j = 0; j < 8; j++) {  // the corners on their own
        float u, v;
        bvhPieceCorner(g, j, u, v);
        for (int k = 0; k < 3; k++) {
          const float q = (v0[k] + u * e1[k]) + v * e2[k];
          if (q < tl[k] || q > th[k]) outside++;
        }
      }
      float lo[3] = {tl[0], tl[1], tl[2]}, hi[3] = {th[0], th[1], th[2]};
      bvhPieceBox(v0, e1, e2, g, lo, hi);
      for (int k = 0; k < 3; k++)
        if (lo[k] < tl[k] || hi[k] > th[k]) {
          if (failures < 5) std::printf("a piece box leaves the five-point box of its triangle: [%a, %a] outside [%a, %a]\n", lo[k], hi[k], tl[k], th[k]);
          failures++;
        }
    }
    std::printf("piece corners outside the five-point box before the intersection: %u\n", outside);
    if (outside == 0) {
      std::printf("the family does not reach its edge\n");
      failures++;
    }
  }

  std::printf("refit edge run finished failures=%d checksum=%08x\n", failures, gSum);
  return failures ? 1 : 0;
}
