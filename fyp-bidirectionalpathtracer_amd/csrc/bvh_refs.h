// bvh_refs.h — the reference stage of the builder (bvh_build.cpp "References"): alpha clipping, split priorities and
// spatial pre-splitting, as ONE text.  The host builder (bvh_build.cpp, alpha_clip.cpp; g++) and the device builder
// (bvh_device.hip k_prio / k_make_refs; hipcc) both compile what is here, so the two make the same pieces, the same boxes
// and the same priorities bit for bit by construction, as they do for bvhQuantiseNode and the refits (bvh.h).  The rules
// of the shared part of bvh.h hold: BVH_HD inline, plain C arithmetic in double precision without contraction (the
// Makefile's -ffp-contract=off), min / max written as the comparisons std::min / std::max make — std::min(a, b) is
// b < a ? b : a, std::max(a, b) is a < b ? b : a: the argument order decides for NaN and signed zeros — and no std::.
#pragma once
#include "bvh.h"

namespace bdpt {

BVH_HD inline double bvhMinD(double a, double b) { return b < a ? b : a; }  // std::min(a, b)
BVH_HD inline double bvhMaxD(double a, double b) { return a < b ? b : a; }  // std::max(a, b)

// ---- geometry -----------------------------------------------------------------------------------------------------
// double -> float rounded outward: the float below / above where the conversion went the other way (nextafterf towards
// -inf / +inf, on the bits: tests/sanitize/san_main.cpp holds the two against std::nextafterf)
BVH_HD inline float bvhFloatDown(double x) {
  float f = (float)x;
  if ((double)f > x) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    u = (f == 0.0f) ? 0x80000001u : ((u & 0x80000000u) ? u + 1u : u - 1u);
    __builtin_memcpy(&f, &u, 4);
  }
  return f;
}
BVH_HD inline float bvhFloatUp(double x) {
  float f = (float)x;
  if ((double)f < x) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    u = (f == 0.0f) ? 0x00000001u : ((u & 0x80000000u) ? u - 1u : u + 1u);
    __builtin_memcpy(&f, &u, 4);
  }
  return f;
}

// Sutherland-Hodgman against the closed half-plane A + B bu + C bv <= 0; `out` holds kBvhPolyMax vertices
BVH_HD inline int bvhClipHalfPlane(const double (*in)[2], int n, double A, double B, double C, double (*out)[2]) {
  int m = 0;
  for (int k = 0; k < n; k++) {
    const double* p = in[k];
    const double* q = in[(k + 1) % n];
    const double fp = A + B * p[0] + C * p[1], fq = A + B * q[0] + C * q[1];
    if (fp <= 0.0 && m < kBvhPolyMax) {
      out[m][0] = p[0];
      out[m][1] = p[1];
      m++;
    }
    if (((fp < 0.0 && fq > 0.0) || (fp > 0.0 && fq < 0.0)) && m < kBvhPolyMax) {
      const double t = fp / (fp - fq);
      out[m][0] = p[0] + t * (q[0] - p[0]);
      out[m][1] = p[1] + t * (q[1] - p[1]);
      m++;
    }
  }
  return m;
}
BVH_HD inline int bvhClipInPlace(double (*poly)[2], int n, double A, double B, double C) {
  double out[kBvhPolyMax][2];
  const int m = bvhClipHalfPlane(poly, n, A, B, C, out);
  for (int k = 0; k < m; k++) {
    poly[k][0] = out[k][0];
    poly[k][1] = out[k][1];
  }
  return m;
}
BVH_HD inline double bvhPolyArea2(const double (*b)[2], int n) {  // twice the area in barycentric units (the whole triangle: 1)
  double s = 0;
  for (int k = 0; k < n; k++) {
    const double* p = b[k];
    const double* q = b[(k + 1) % n];
    s += p[0] * q[1] - q[0] * p[1];
  }
  return fabs(s);
}
// The box of the polygon's points v0 + bu e1 + bv e2, rounded outward to float, intersected with an outer box.
// (lo, hi) must not alias the outer box.
BVH_HD inline void bvhPolyBoxIn(const BvhTri& r, const double (*b)[2], int n, const float* outerLo, const float* outerHi, float* lo, float* hi) {
  double dlo[3] = {1e300, 1e300, 1e300}, dhi[3] = {-1e300, -1e300, -1e300};
  for (int k = 0; k < n; k++)
    for (int a = 0; a < 3; a++) {
      const double p = (double)r.v0[a] + b[k][0] * (double)r.e1[a] + b[k][1] * (double)r.e2[a];
      dlo[a] = bvhMinD(dlo[a], p);
      dhi[a] = bvhMaxD(dhi[a], p);
    }
  for (int a = 0; a < 3; a++) {
    const float pl = bvhFloatDown(dlo[a]), ph = bvhFloatUp(dhi[a]);
    lo[a] = pl < outerLo[a] ? outerLo[a] : pl;  // std::max(pl, outerLo)
    hi[a] = outerHi[a] < ph ? outerHi[a] : ph;  // std::min(ph, outerHi)
    if (hi[a] < lo[a]) hi[a] = lo[a];           // (outward rounding of two disjoint-by-an-ulp intervals)
  }
}

struct BvhSplitGrid {  // spatial-median planes of the scene box on a 2^30 grid per axis
  double lo[3], ext[3];
  // most important plane strictly inside [a, b] on `axis`: its importance (bit position, higher = nearer the root) or -1
  BVH_HD int plane(int axis, float a, float b, double& coord) const {
    if (!(ext[axis] > 0.0) || !(b > a)) return -1;
    const double s = 1073741824.0 / ext[axis];
    double ua = floor(((double)a - lo[axis]) * s), ub = floor(((double)b - lo[axis]) * s);
    ua = bvhMinD(bvhMaxD(ua, 0.0), 1073741823.0);
    ub = bvhMinD(bvhMaxD(ub, 0.0), 1073741823.0);
    const uint32_t ia = (uint32_t)ua, ib = (uint32_t)ub;
    if (ia == ib) return -1;
    const uint32_t diff = ia ^ ib;
    const int h = 31 - __builtin_clz(diff);
    const uint32_t pl = (ib >> h) << h;
    coord = lo[axis] + (double)pl / s;
    if (!(coord > (double)a && coord < (double)b)) return -1;  // (rounding at the ends of the interval)
    return h;
  }
  BVH_HD int dominant(const float* blo, const float* bhi, int& axis, double& coord) const {
    int best = -1;
    float bestExt = -1.0f;
    for (int a = 0; a < 3; a++) {
      double c = 0.0;
      const int h = plane(a, blo[a], bhi[a], c);
      const float e = bhi[a] - blo[a];
      if (h > best || (h == best && h >= 0 && e > bestExt)) {
        best = h;
        bestExt = e;
        axis = a;
        coord = c;
      }
    }
    return best;
  }
};

// (2^-level (A_box - A_ideal))^(1/3): bvh_build.cpp "References".  polyShare: the part of the triangle the box bounds.
BVH_HD inline double bvhSplitPriority(const BvhSplitGrid& G, const BvhTri& r, const float* lo, const float* hi, double polyShare) {
  int axis = 0;
  double c = 0;
  const int h = G.dominant(lo, hi, axis, c);
  if (h < 0) return 0.0;
  const double cx = (double)r.e1[1] * r.e2[2] - (double)r.e1[2] * r.e2[1], cy = (double)r.e1[2] * r.e2[0] - (double)r.e1[0] * r.e2[2],
               cz = (double)r.e1[0] * r.e2[1] - (double)r.e1[1] * r.e2[0];
  const double ideal = (fabs(cx) + fabs(cy) + fabs(cz)) * polyShare;
  const double dx = (double)hi[0] - lo[0], dy = (double)hi[1] - lo[1], dz = (double)hi[2] - lo[2];
  const double gain = 2.0 * (dx * dy + dy * dz + dz * dx) - ideal;
  if (!(gain > 0.0)) return 0.0;
  return bvhCbrt(ldexp(gain, h - 30));
}

// ---- a piece of a triangle: a convex polygon in its barycentric plane, the splits it may still get, its box ----------
// (Pieces are copied whole, b[n ..] and a `splits` not yet set included: those are never read before they are written.)
struct BvhPiece {
  double b[kBvhPolyMax][2];
  int n;
  uint32_t splits;
  float lo[3], hi[3];
};

// ---- the alpha clip on plain tables (what BvhClipTables holds, as pointers: the clipper's own arrays on the host,
// copies of them on the device) --------------------------------------------------------------------------------------
struct BvhClipMask {
  int32_t w, h;
  const uint32_t* sat;  // summed-area table, (w + 1) x (h + 1): cells a sample may pass in
};
struct BvhClipView {
  const uint32_t* triMaterial;  // per triangle
  const uint32_t* indices;      // 3 per triangle
  const float* texcoords;       // 3 floats per vertex, or null
  const int32_t* matMask;       // per material: index into masks, -1: no texture decides
  const int32_t* matVerdict;    // for matMask < 0: 1 the test always passes, 2 it always fails
  const BvhClipMask* masks;
};
BVH_HD inline int64_t bvhFloorDiv(int64_t a, int64_t n) {
  int64_t q = a / n;
  if ((a % n) != 0 && ((a < 0) != (n < 0))) q--;
  return q;
}
// marked cells in [x0, x1] x [y0, y1] of the w x h table `sat`: unwrapped inclusive coordinates, each span at most one
// period long
BVH_HD inline uint32_t bvhClipCount(const uint32_t* sat, int32_t w, int32_t h, int64_t x0, int64_t x1, int64_t y0, int64_t y1) {
  if (x1 < x0 || y1 < y0) return 0;
  const size_t W1 = (size_t)w + 1;
  int64_t xs[2][2], ys[2][2];
  int nx = 0, ny = 0;
  {
    const int64_t s = bvhFloorDiv(x0, w) * w, a = x0 - s, b = x1 - s;
    if (b < w) {
      xs[nx][0] = a, xs[nx][1] = b, nx++;
    } else {
      xs[nx][0] = a, xs[nx][1] = w - 1, nx++;
      xs[nx][0] = 0, xs[nx][1] = (b - w) < (int64_t)(w - 1) ? (b - w) : (int64_t)(w - 1), nx++;
    }
  }
  {
    const int64_t s = bvhFloorDiv(y0, h) * h, a = y0 - s, b = y1 - s;
    if (b < h) {
      ys[ny][0] = a, ys[ny][1] = b, ny++;
    } else {
      ys[ny][0] = a, ys[ny][1] = h - 1, ny++;
      ys[ny][0] = 0, ys[ny][1] = (b - h) < (int64_t)(h - 1) ? (b - h) : (int64_t)(h - 1), ny++;
    }
  }
  uint32_t c = 0;
  for (int i = 0; i < nx; i++)
    for (int j = 0; j < ny; j++) {
      const int64_t xa = xs[i][0], xb = xs[i][1], ya = ys[j][0], yb = ys[j][1];  // wrapped-in-range inclusive
      c += sat[((size_t)yb + 1) * W1 + (size_t)xb + 1] - sat[(size_t)ya * W1 + (size_t)xb + 1] - sat[((size_t)yb + 1) * W1 + (size_t)xa] +
           sat[(size_t)ya * W1 + (size_t)xa];
    }
  return c;
}
// The cells the samples of a barycentric polygon of triangle `tri` can fall in, a span of a whole period or more set to
// [0, w - 1] / [0, h - 1] (fullX / fullY).  Returns false when nothing can be said (no texture coordinates, non-finite
// or huge ones).
struct BvhCellRect {
  int64_t x0, x1, y0, y1;
  bool fullX, fullY;
  double margin;
  double uv[3][2];  // the triangle's texture coordinates
};
BVH_HD inline bool bvhClipCellRect(const BvhClipView& V, const BvhClipMask& m, uint32_t tri, const double (*poly)[2], int n, BvhCellRect& R) {
  if (!V.texcoords) return false;
  double big = 0.0;
  for (int k = 0; k < 3; k++) {
    const uint32_t vi = V.indices[(size_t)tri * 3 + (size_t)k];
    R.uv[k][0] = (double)V.texcoords[(size_t)vi * 3];
    R.uv[k][1] = (double)V.texcoords[(size_t)vi * 3 + 1];
    if (!__builtin_isfinite(R.uv[k][0]) || !__builtin_isfinite(R.uv[k][1])) return false;
    big = bvhMaxD(big, bvhMaxD(fabs(R.uv[k][0]), fabs(R.uv[k][1])));
  }
  if (big > 4096.0) return false;
  // What separates the texel the device's alpha test samples from the one under the exact hit point: the fp32
  // rounding of the coordinate itself (a few ulps of its magnitude) and, for rays that graze the triangle, the error of
  // the Moeller-Trumbore barycentrics (eps * distance / (extent * sin of the incidence angle)).  Half a texel covers
  // the second down to a fraction of a degree for a card a few hundred texels across — the same order of world-space
  // slack as the pad every box of the tree gets (bvh_build.cpp: 2e-5 of the scene diagonal).
  R.margin = 0.5 + 1e-5 * (big + 1.0) * (double)(m.w < m.h ? m.h : m.w);
  double xa = 1e300, xb = -1e300, ya = 1e300, yb = -1e300;
  for (int k = 0; k < n; k++) {
    const double b0 = 1.0 - poly[k][0] - poly[k][1];
    const double u = R.uv[0][0] * b0 + R.uv[1][0] * poly[k][0] + R.uv[2][0] * poly[k][1];
    const double v = R.uv[0][1] * b0 + R.uv[1][1] * poly[k][0] + R.uv[2][1] * poly[k][1];
    const double x = u * (double)m.w - 0.5, y = v * (double)m.h - 0.5;
    xa = bvhMinD(xa, x);
    xb = bvhMaxD(xb, x);
    ya = bvhMinD(ya, y);
    yb = bvhMaxD(yb, y);
  }
  R.x0 = (int64_t)floor(xa - R.margin), R.x1 = (int64_t)floor(xb + R.margin);
  R.y0 = (int64_t)floor(ya - R.margin), R.y1 = (int64_t)floor(yb + R.margin);
  R.fullX = R.x1 - R.x0 + 1 >= m.w, R.fullY = R.y1 - R.y0 + 1 >= m.h;
  if (R.fullX) R.x0 = 0, R.x1 = m.w - 1;
  if (R.fullY) R.y0 = 0, R.y1 = m.h - 1;
  return true;
}
// One end of the smallest rectangle of cells that holds every cell of R a sample may pass in (there is one): the
// first (FIRST) or the last column (COLS) or row that has such a cell, by bisection on the count of the strip from
// that end of R.
template <bool COLS, bool FIRST>
BVH_HD inline int64_t bvhClipEdge(const BvhClipMask& m, const BvhCellRect& R) {
  int64_t a = COLS ? R.x0 : R.y0, b = COLS ? R.x1 : R.y1;
  while (a < b) {
    const int64_t mid = a + (b - a + (FIRST ? 0 : 1)) / 2;
    const int64_t s0 = FIRST ? (COLS ? R.x0 : R.y0) : mid, s1 = FIRST ? mid : (COLS ? R.x1 : R.y1);
    const bool any = (COLS ? bvhClipCount(m.sat, m.w, m.h, s0, s1, R.y0, R.y1) : bvhClipCount(m.sat, m.w, m.h, R.x0, R.x1, s0, s1)) > 0;
    if (FIRST) {
      if (any)
        b = mid;
      else
        a = mid + 1;
    } else {
      if (any)
        a = mid;
      else
        b = mid - 1;
    }
  }
  return a;
}
// BvhRefClipper::clip on the tables: shrinks the polygon to where the alpha test of triangle `tri` can pass; false when
// nothing is left.
BVH_HD inline bool bvhClipPoly(const BvhClipView& V, uint32_t tri, double (*poly)[2], int& n) {
  const uint32_t mat = V.triMaterial[tri];
  const int32_t mask = V.matMask[mat];
  if (mask < 0) return V.matVerdict[mat] != 2;
  const BvhClipMask m = V.masks[mask];
  BvhCellRect R;
  if (!bvhClipCellRect(V, m, tri, poly, n, R)) return true;
  if (bvhClipCount(m.sat, m.w, m.h, R.x0, R.x1, R.y0, R.y1) == 0) return false;
  // a sample falls in cell floor(x), x = u w - 0.5 as the device computes it: cells [c0, c1] <=> x in [c0, c1 + 1)
  const double du1 = R.uv[1][0] - R.uv[0][0], du2 = R.uv[2][0] - R.uv[0][0], dv1 = R.uv[1][1] - R.uv[0][1], dv2 = R.uv[2][1] - R.uv[0][1];
  if (!R.fullX) {
    const int64_t c0 = bvhClipEdge<true, true>(m, R), c1 = bvhClipEdge<true, false>(m, R);
    const double uLo = ((double)c0 + 0.5 - R.margin) / (double)m.w, uHi = ((double)c1 + 1.5 + R.margin) / (double)m.w;
    if (c0 > R.x0) n = bvhClipInPlace(poly, n, uLo - R.uv[0][0], -du1, -du2);              // u >= uLo
    if (n >= 3 && c1 < R.x1) n = bvhClipInPlace(poly, n, R.uv[0][0] - uHi, du1, du2);      // u <= uHi
  }
  if (n >= 3 && !R.fullY) {
    const int64_t r0 = bvhClipEdge<false, true>(m, R), r1 = bvhClipEdge<false, false>(m, R);
    const double vLo = ((double)r0 + 0.5 - R.margin) / (double)m.h, vHi = ((double)r1 + 1.5 + R.margin) / (double)m.h;
    if (r0 > R.y0) n = bvhClipInPlace(poly, n, vLo - R.uv[0][1], -dv1, -dv2);
    if (n >= 3 && r1 < R.y1) n = bvhClipInPlace(poly, n, R.uv[0][1] - vHi, dv1, dv2);
  }
  return n >= 3;
}

// ---- the work per triangle.  Clip: bool(double (*poly)[2], int& n), the triangle's clipper (the host: the virtual
// BvhRefClipper::clip; the device: bvhClipPoly); only called where `alpha` says the triangle is clipped at all ---------
// The whole triangle (box tlo, thi) as a piece, shrunk by the clipper.  false: nothing of it can be hit.
template <class Clip>
BVH_HD inline bool bvhWholePiece(const BvhTri& r, const float* tlo, const float* thi, bool alpha, const Clip& clip, BvhPiece& pc, bool& shrunk) {
  pc.n = 3;
  pc.b[0][0] = 0.0;
  pc.b[0][1] = 0.0;
  pc.b[1][0] = 1.0;
  pc.b[1][1] = 0.0;
  pc.b[2][0] = 0.0;
  pc.b[2][1] = 1.0;
  pc.splits = 0;
  for (int a = 0; a < 3; a++) {
    pc.lo[a] = tlo[a];
    pc.hi[a] = thi[a];
  }
  shrunk = false;
  if (!alpha) return true;
  if (!clip(pc.b, pc.n) || pc.n < 3) return false;
  shrunk = !(pc.n == 3 && pc.b[0][0] == 0.0 && pc.b[0][1] == 0.0 && pc.b[1][0] == 1.0 && pc.b[1][1] == 0.0 && pc.b[2][0] == 0.0 && pc.b[2][1] == 1.0);
  if (shrunk) bvhPolyBoxIn(r, pc.b, pc.n, tlo, thi, pc.lo, pc.hi);
  return true;
}
// Pass 1 for one triangle: what the clipper leaves of it (state: 0 = plain reference (its box), 1 = shrunk by the
// clipper, 2 = dropped), its split priority and the most splits it may get.
template <class Clip>
BVH_HD inline void bvhRefDecide(const BvhSplitGrid& G, const BvhTri& r, const float* tlo, const float* thi, bool haveClipper, const Clip& clip,
                                float budgetOpaque, float budgetAlpha, float outlierArea, uint8_t& state, double& prio, float& cap) {
  prio = 0.0;
  cap = (float)BDPT_SPLIT_MAX_PER_TRI;
  const bool nonOpaque = (r.flags & kTriNonOpaque) != 0;
  BvhPiece pc;
  bool shrunk = false;
  if (!bvhWholePiece(r, tlo, thi, nonOpaque && haveClipper, clip, pc, shrunk)) {
    state = 2;
    return;
  }
  state = shrunk ? 1 : 0;
  const float budget = nonOpaque ? budgetAlpha : budgetOpaque;
  const float area = bvhBoxArea(pc.lo, pc.hi);
  if (budget > 0.0f && (nonOpaque || area >= outlierArea)) {
    prio = bvhSplitPriority(G, r, pc.lo, pc.hi, shrunk ? bvhPolyArea2(pc.b, pc.n) : 1.0);
    // an opaque outlier is cut down to about the size of its neighbours, not further
    if (!nonOpaque && outlierArea > 0.0f) {
      const float f = floorf((float)BDPT_SPLIT_OUTLIER * area / outlierArea);
      cap = f < (float)BDPT_SPLIT_MAX_PER_TRI ? f : (float)BDPT_SPLIT_MAX_PER_TRI;  // std::min(MAX, f)
    }
  }
}
// All references of one triangle, in a fixed order: the piece pc (pc.splits > 0; clobbered) cut at the dominant plane
// of its box until its splits are used up, every half clipped again, emit(piece) for every piece that stays.  `stack`
// holds pc.splits pieces (a piece is stacked once per split that succeeds).
template <class Clip, class Emit>
BVH_HD inline void bvhSplitTriangle(const BvhSplitGrid& G, const BvhTri& r, BvhPiece& pc, bool alpha, BvhPiece* stack, const Clip& clip, const Emit& emit) {
  uint32_t sp = 0;
  for (;;) {
    for (int guard = 0;; guard++) {
      int axis = 0;
      double c = 0;
      if (pc.splits == 0 || guard > 96 || pc.n + 2 > kBvhPolyMax || G.dominant(pc.lo, pc.hi, axis, c) < 0) {
        emit(pc);
        break;
      }
      const double PA = (double)r.v0[axis] - c, PB = (double)r.e1[axis], PC = (double)r.e2[axis];
      BvhPiece lo, hi;
      lo.n = bvhClipHalfPlane(pc.b, pc.n, PA, PB, PC, lo.b);
      hi.n = bvhClipHalfPlane(pc.b, pc.n, -PA, -PB, -PC, hi.b);
      bool haveLo = lo.n >= 3 && bvhPolyArea2(lo.b, lo.n) > 0.0, haveHi = hi.n >= 3 && bvhPolyArea2(hi.b, hi.n) > 0.0;
      if (alpha) {
        if (haveLo) haveLo = clip(lo.b, lo.n) && lo.n >= 3;
        if (haveHi) haveHi = clip(hi.b, hi.n) && hi.n >= 3;
      }
      if (haveLo) bvhPolyBoxIn(r, lo.b, lo.n, pc.lo, pc.hi, lo.lo, lo.hi);
      if (haveHi) bvhPolyBoxIn(r, hi.b, hi.n, pc.lo, pc.hi, hi.lo, hi.hi);
      if (!haveLo && !haveHi) {
        if (!alpha) emit(pc);  // (a sliver the clip lost to rounding: keep the piece as it was)
        break;
      }
      if (!haveLo || !haveHi) {  // the polygon lies on one side of the plane although its box straddles it: shrink and go on
        const uint32_t s = pc.splits;
        pc = haveLo ? lo : hi;
        pc.splits = s;
        continue;
      }
      const uint32_t rest = pc.splits - 1;
      const double wl = ((double)lo.hi[0] - lo.lo[0]) + ((double)lo.hi[1] - lo.lo[1]) + ((double)lo.hi[2] - lo.lo[2]);
      const double wh = ((double)hi.hi[0] - hi.lo[0]) + ((double)hi.hi[1] - hi.lo[1]) + ((double)hi.hi[2] - hi.lo[2]);
      uint32_t sl = (wl + wh > 0.0) ? (uint32_t)floor((double)rest * wl / (wl + wh) + 0.5) : rest / 2;
      if (sl > rest) sl = rest;
      lo.splits = sl;
      hi.splits = rest - sl;
      stack[sp++] = hi;
      pc = lo;
      guard = 0;
    }
    if (sp == 0) break;
    pc = stack[--sp];
  }
}

// ---- host only: the split scale of a class, the largest D with total(D) = sum min(floor(D p_t), cap_t) <= budget ------
// pmax: the class's largest priority (> 0).  total(D) is the caller's sum (integers: independent of how it is shared out).
template <class Total>
inline double bvhSplitScale(double pmax, uint64_t budget, const Total& total) {
  double dLo = 0.0, dHi = ((double)BDPT_SPLIT_MAX_PER_TRI + 1.0) / pmax;  // at dHi the largest priority is capped
  if (total(dHi) <= budget) return dHi;
  for (int it = 0; it < 40; it++) {
    const double mid = 0.5 * (dLo + dHi);
    if (total(mid) <= budget)
      dLo = mid;
    else
      dHi = mid;
  }
  return dLo;
}

}  // namespace bdpt
