// bvh_build.cpp — binned-SAH top-down builder producing the flat 64-byte-node layout of bvh.h.
//
// Threaded (std::thread): the top of the tree is split by one thread with the binning of large nodes shared
// among all, then the subtrees below a grain size are built concurrently on disjoint ranges of the
// triangle order; the per-triangle and per-node passes run as parallel loops.  The result does not depend on
// the thread count, bit for bit: bin bounds and counts are order-independent (min / max / integer sums), every
// partition is the same serial std::partition on the same range, the four-wide collapse only looks at the tree's
// shape, and the one floating-point sum (the SAH cost) is taken in node order by one thread.
#include "bvh.h"
#include "bvh_refs.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <mutex>
#include <thread>

#include <sched.h>

namespace bdpt {
namespace {

using Box = BvhBox;            // bvh.h: shared with the device-side tree builder
using TmpNode = BvhBuildNode;  // the binary tree: children always behind their parent
inline TmpNode makeTmpNode(uint32_t first, uint32_t count, uint32_t depth) {
  TmpNode n;
  n.box.reset();
  n.left = n.right = -1;
  n.first = first;
  n.count = count;
  n.depth = depth;
  return n;
}

#ifndef BDPT_SAH_BINS
#define BDPT_SAH_BINS 16
#endif
#ifndef BDPT_LEAF_MAX
#define BDPT_LEAF_MAX 2
#endif
// Default budgets.  Opaque triangles: none — measured on the bench atrium (tools/bvh_eval.py, profiles/README.md r3)
// pre-splitting by priority makes an evenly tessellated scene's tree worse at every setting tried (SAH cost 31.3 ->
// 31.5-35.2, +0-14 % node visits); the knob (also the environment variable BDPT_SPLIT_BUDGET) stays for scenes that
// mix huge and tiny triangles.  Non-opaque triangles: four extra references each — the 10 M-triangle
// courtyard's closest-hit rays go from 76 node visits + 55 triangle tests to 40 + 12 and its 4K depth-16 frame from 905 ms to
// 373 ms (budgets 2 / 4 / 8: 435 / 373 / 361 ms at 7 / 13 / 16 s of scene set-up).
#ifndef BDPT_SPLIT_BUDGET
#define BDPT_SPLIT_BUDGET 0.0f
#endif
#ifndef BDPT_SPLIT_BUDGET_ALPHA
#define BDPT_SPLIT_BUDGET_ALPHA 4.0f
#endif
constexpr int kBins = kBvhBins;
constexpr uint32_t kStablePartitionMin = 1u << 16;  // nodes of at least this many references are partitioned stably, in parallel
constexpr size_t kPartitionChunk = 1u << 14;
constexpr uint32_t kCollapseGrain = 1u << 15;  // binary subtrees of at most this many nodes are collapsed to four-wide nodes by one worker each
// Leaves hold at most two triangles.  Measured on the bench frame (profiles/README.md r2): leaves of <= 1 / 2 / 3 / 4 / 8
// triangles give 23.6 / 19.1 / 19.5 / 20.1 / 23.0 ms per frame — a triangle test costs half a node visit and leaf runs of
// different lengths idle lanes, while one-triangle leaves double the node array past the 4 MiB L2 of an XCD.
constexpr uint32_t kLeafMax = kBvhLeafMax;
constexpr float kCostTraverse = 1.0f, kCostTri = 1.0f;
constexpr int kBinaryMaxDepth = kBvhBinaryMaxDepth;  // depth budget of the intermediate binary tree: a two-wide path stacks one reference per level, so the device stack bounds it (a budget of 48 let a 10 M-triangle scene of overlapping cards through that bdpt_set_scene then had to refuse)

inline uint32_t ceilLog2(uint32_t x) {
  uint32_t l = 0;
  while ((1u << l) < x) l++;
  return l;
}

// [0, n) in `threads` contiguous chunks, one std::thread each (the caller's thread takes chunk 0)
template <class F>
void parallelFor(size_t n, int threads, const F& f) {
  if (threads <= 1 || n < 4096) {
    f((size_t)0, n, 0);
    return;
  }
  WorkerScope pool;
  const size_t chunk = (n + (size_t)threads - 1) / (size_t)threads;
  for (int t = 1; t < threads; t++) {
    const size_t a = std::min(n, chunk * (size_t)t), b = std::min(n, a + chunk);
    if (a < b) pool.spawn([&f, a, b, t] { f(a, b, t); });
  }
  f((size_t)0, std::min(n, chunk), 0);
  pool.join();
}

// [0, n) in chunks of `chunk` items handed out through an atomic counter (work per item may differ by orders of
// magnitude: a split triangle against an untouched one); f(chunkIndex, first, last).  What a chunk produces must only
// depend on its index, so that results assembled in chunk order do not depend on the thread count.
template <class F>
void parallelChunks(size_t n, int threads, size_t chunk, const F& f) {
  const size_t numChunks = (n + chunk - 1) / chunk;
  if (threads <= 1 || numChunks <= 1) {
    for (size_t c = 0; c < numChunks; c++) f(c, c * chunk, std::min(n, (c + 1) * chunk));
    return;
  }
  std::atomic<size_t> next{0};
  auto worker = [&] {
    for (;;) {
      const size_t c = next.fetch_add(1);
      if (c >= numChunks) return;
      f(c, c * chunk, std::min(n, (c + 1) * chunk));
    }
  };
  WorkerScope pool;
  for (int t = 1; t < threads; t++) pool.spawn(worker);
  worker();
  pool.join();
}

// What the tree is built over: one 40-byte record per reference — the box of the piece it stands for, the box's
// centre, and its index in the reference list.  The records THEMSELVES are permuted as nodes are partitioned (round 4;
// before, an index array was permuted and every scan of a node gathered boxes and centres through it): every pass over
// a node — bounds, binning, the partition — then streams a contiguous range instead of gathering 36 bytes per element
// from a gigabyte of boxes, which is what bounded the builder on 16 host threads.
using Ref = BvhBuildRef;

struct BuildData {
  BigVec<Ref>& refs;     // permuted in place: a node owns a contiguous range
  BigVec<Ref>& scratch;  // as large as refs: the stable partition of large nodes scatters through it
};

struct Bins {
  Box bb[3][kBins];
  uint32_t bc[3][kBins];
  void reset() {
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < kBins; b++) {
        bb[a][b].reset();
        bc[a][b] = 0;
      }
  }
};

// Bounds of a node and the position of its split (0 = leaf).  `threads` > 1 shares the two O(count) scans.
uint32_t splitNode(const BuildData& B, uint32_t first, uint32_t count, uint32_t depth, int threads, Box& nodeBox) {
  Ref* const base = B.refs.data() + first;
  Box nb, cb;
  nb.reset();
  cb.reset();
  if (threads > 1 && count >= (1u << 16)) {
    std::vector<Box> pn((size_t)threads), pc((size_t)threads);
    for (int t = 0; t < threads; t++) {
      pn[(size_t)t].reset();
      pc[(size_t)t].reset();
    }
    parallelFor(count, threads, [&](size_t a, size_t b, int t) {
      Box n0, c0;
      n0.reset();
      c0.reset();
      for (size_t k = a; k < b; k++) {
        n0.grow(base[k].box);
        c0.grow(base[k].cent);
      }
      pn[(size_t)t] = n0;
      pc[(size_t)t] = c0;
    });
    for (int t = 0; t < threads; t++) {
      nb.grow(pn[(size_t)t]);
      cb.grow(pc[(size_t)t]);
    }
  } else {
    for (uint32_t k = 0; k < count; k++) {
      nb.grow(base[k].box);
      cb.grow(base[k].cent);
    }
  }
  nodeBox = nb;
  if (count <= kLeafMax) return 0;

  // Depth budget: once the remaining levels are only just enough for a balanced split of
  // `count` triangles into leaves, stop trusting SAH and split at the median.
  const bool forceMedian = depth + ceilLog2((count + kLeafMax - 1) / kLeafMax) + 1 >= (uint32_t)kBinaryMaxDepth;

  int bestAxis = -1, bestSplit = -1;
  float bestCost = 1e30f;
  if (!forceMedian) {
    float lo[3], scale[3];
    bool use[3];
    for (int axis = 0; axis < 3; axis++) {
      const float ext = cb.hi[axis] - cb.lo[axis];
      lo[axis] = cb.lo[axis];
      use[axis] = ext > 0.0f;
      scale[axis] = use[axis] ? (float)kBins / ext : 0.0f;
    }
    auto binRange = [&](size_t a, size_t b, Bins& bins) {
      for (size_t k = a; k < b; k++) {
        const Ref& r = base[k];
        for (int axis = 0; axis < 3; axis++) {
          if (!use[axis]) continue;
          int bi = (int)((r.cent[axis] - lo[axis]) * scale[axis]);
          bi = std::min(std::max(bi, 0), kBins - 1);
          bins.bb[axis][bi].grow(r.box);
          bins.bc[axis][bi]++;
        }
      }
    };
    Bins bins;
    bins.reset();
    if (threads > 1 && count >= (1u << 16)) {
      std::vector<Bins> part((size_t)threads);
      for (Bins& pb : part) pb.reset();
      parallelFor(count, threads, [&](size_t a, size_t b, int t) { binRange(a, b, part[(size_t)t]); });
      for (const Bins& pb : part)
        for (int axis = 0; axis < 3; axis++)
          for (int b = 0; b < kBins; b++) {
            bins.bb[axis][b].grow(pb.bb[axis][b]);
            bins.bc[axis][b] += pb.bc[axis][b];
          }
    } else {
      binRange(0, count, bins);
    }
    for (int axis = 0; axis < 3; axis++) {
      if (!use[axis]) continue;
      const Box* bb = bins.bb[axis];
      const uint32_t* bc = bins.bc[axis];
      float rightArea[kBins];
      uint32_t rightCnt[kBins];
      Box acc;
      acc.reset();
      uint32_t cnt = 0;
      for (int b = kBins - 1; b > 0; b--) {
        acc.grow(bb[b]);
        cnt += bc[b];
        rightArea[b] = acc.area();
        rightCnt[b] = cnt;
      }
      acc.reset();
      cnt = 0;
      for (int b = 0; b < kBins - 1; b++) {
        acc.grow(bb[b]);
        cnt += bc[b];
        if (cnt == 0 || rightCnt[b + 1] == 0) continue;
        const float cost = acc.area() * (float)cnt + rightArea[b + 1] * (float)rightCnt[b + 1];
        if (cost < bestCost) {
          bestCost = cost;
          bestAxis = axis;
          bestSplit = b;
        }
      }
    }
  }
  // A STABLE partition of the node's range — lefts in their order, then rights in theirs — is the one way references
  // move, whatever decides who goes left.  Large nodes (the top of the tree: a few dozen nodes that together touch every
  // reference several times) do it in three parallel passes: count the lefts of every chunk, scatter the records into
  // the scratch array at offsets from those counts, copy back.  The chunks are fixed-size, not per-thread, and the rule is
  // chosen by the node's SIZE, so the permutation — and with it the tree — does not depend on the thread count; small
  // nodes do the same by one thread.  One rule for every node size: a builder that partitions in parallel — the passes
  // here, or a device (bvh_device.hip: flags, scan, scatter) — produces the very same permutation.
  auto partitionStable = [&](auto&& goesLeft) -> uint32_t {
    Ref* const tmp = B.scratch.data() + first;
    if (count >= kStablePartitionMin) {
      const size_t nChunks = ((size_t)count + kPartitionChunk - 1) / kPartitionChunk;
      std::vector<uint32_t> lefts(nChunks + 1, 0);
      parallelChunks(count, threads, kPartitionChunk, [&](size_t ci, size_t a, size_t b) {
        uint32_t n = 0;
        for (size_t k = a; k < b; k++) n += goesLeft(base[k]) ? 1u : 0u;
        lefts[ci + 1] = n;
      });
      for (size_t ci = 0; ci < nChunks; ci++) lefts[ci + 1] += lefts[ci];
      const uint32_t nLeft = lefts[nChunks];
      parallelChunks(count, threads, kPartitionChunk, [&](size_t ci, size_t a, size_t b) {
        uint32_t l = lefts[ci], r = nLeft + ((uint32_t)a - lefts[ci]);
        for (size_t k = a; k < b; k++) {
          if (goesLeft(base[k]))
            tmp[l++] = base[k];
          else
            tmp[r++] = base[k];
        }
      });
      parallelChunks(count, threads, kPartitionChunk, [&](size_t, size_t a, size_t b) { std::memcpy(base + a, tmp + a, (b - a) * sizeof(Ref)); });
      return nLeft;
    }
    uint32_t l = 0, r = 0;
    for (uint32_t k = 0; k < count; k++) {
      if (goesLeft(base[k]))
        base[l++] = base[k];  // (l <= k: never overwrites an element not yet read)
      else
        tmp[r++] = base[k];
    }
    std::memcpy(base + l, tmp, (size_t)r * sizeof(Ref));
    return l;
  };
  uint32_t mid = 0;
  if (bestAxis >= 0) {
    const float lo = cb.lo[bestAxis], ext = cb.hi[bestAxis] - cb.lo[bestAxis];
    const float scale = (float)kBins / ext;
    mid = partitionStable([&](const Ref& r) {
      int b = (int)((r.cent[bestAxis] - lo) * scale);
      b = std::min(std::max(b, 0), kBins - 1);
      return b <= bestSplit;
    });
  }
  if (mid == 0 || mid == count) {
    // Median split on the widest centroid axis (also the degenerate all-equal case): the count / 2 references that come
    // first by (centroid, reference id) go left — found by SELECTING the pivot, not by sorting — and the same stable
    // partition moves them: no order inside the halves has to be defined beyond the one they already have, and a device
    // does it with a radix select and the partition machinery it has anyway.
    int axis = 0;
    const float e0 = cb.hi[0] - cb.lo[0], e1 = cb.hi[1] - cb.lo[1], e2 = cb.hi[2] - cb.lo[2];
    if (e1 > e0 && e1 >= e2) axis = 1;
    if (e2 > e0 && e2 > e1) axis = 2;
    std::vector<std::pair<float, uint32_t>> keys(count);
    for (uint32_t k = 0; k < count; k++) keys[k] = {base[k].cent[axis], base[k].id};
    std::nth_element(keys.begin(), keys.begin() + count / 2, keys.end());
    const std::pair<float, uint32_t> pivot = keys[count / 2];
    mid = partitionStable([&](const Ref& r) { return std::pair<float, uint32_t>(r.cent[axis], r.id) < pivot; });
  }
  return mid;
}

// Whole subtree under nodes[root] (its first / count / depth already set), depth first, appended to `nodes`.
// Children are always created after their parent.
void buildSubtree(const BuildData& B, BigVec<TmpNode>& nodes, uint32_t root, uint32_t splitBelow, int threads,
                  std::vector<uint32_t>* deferred) {
  std::vector<uint32_t> todo{root};
  while (!todo.empty()) {
    const uint32_t ni = todo.back();
    todo.pop_back();
    const uint32_t first = nodes[ni].first, count = nodes[ni].count, depth = nodes[ni].depth;
    if (deferred && ni != root && count <= splitBelow) {  // small enough: some thread builds it later
      deferred->push_back(ni);
      continue;
    }
    Box nb;
    const uint32_t mid = splitNode(B, first, count, depth, threads, nb);
    nodes[ni].box = nb;
    if (mid == 0) continue;
    const TmpNode l = makeTmpNode(first, mid, depth + 1), r = makeTmpNode(first + mid, count - mid, depth + 1);
    const uint32_t li = (uint32_t)nodes.size();
    nodes.push_back(l);
    nodes.push_back(r);
    nodes[ni].left = (int32_t)li;
    nodes[ni].right = (int32_t)li + 1;
    nodes[ni].count = 0;
    todo.push_back(li + 1);
    todo.push_back(li);
  }
}


// ------------------------------------------------------------------------------------------------
// References.  The tree is built over REFERENCES, not triangles: a reference is (triangle, box of the piece of it
// the reference stands for).  One reference per triangle gives the classic object-split tree; spatial
// pre-splitting cuts the box of a triangle at spatial-median planes of the scene box and gives every piece its own
// reference, so that large or diagonal triangles (and, above all, the overlapping alpha-masked cards of foliage)
// stop inflating every box above them.  The leaf still intersects the WHOLE triangle (device_trace.hpp triGeom): a
// hit found through any reference of a triangle is that triangle's one hit, and the closest-hit tie rule (lowest
// primitive index; the same primitive never replaces itself) makes duplicates harmless.
//
// How many splits a triangle gets follows Karras & Aila, "Fast parallel construction of high-quality bounding
// volume hierarchies" (HPG 2013), section 4.3: priority p = (2^-level * (A_box - A_ideal))^(1/3), where level is
// that of the most important spatial-median plane cutting the box and A_ideal = |e1 x e2|_1 is the box area the
// triangle would reach if split without end; split counts s_t = floor(D p_t) with D chosen so that their sum meets
// the budget; a piece hands its remaining splits to its two halves in proportion to their extents.
//
// Pieces are convex polygons in the triangle's barycentric plane (vertex = (bu, bv), P = v0 + bu e1 + bv e2),
// clipped in double precision; a piece's box is rounded outwards to float (the builder's pad covers the fp32
// rounding of the device's triangle test, as it does for whole triangles).  For non-opaque triangles the caller's
// BvhRefClipper shrinks a piece to where the alpha test can pass, or drops it.
// ------------------------------------------------------------------------------------------------
// The arithmetic of all this — clipping, boxes, the split grid, priorities, bvhSplitTriangle — is bvh_refs.h, the one text
// the device builder (bvh_device.hip) compiles too; what follows here only loads, calls and stores.
struct RefOut {
  std::vector<Box> boxes;
  std::vector<uint32_t> tri;
  void push(const float* lo, const float* hi, uint32_t t) {
    Box bx;
    for (int a = 0; a < 3; a++) {
      bx.lo[a] = lo[a];
      bx.hi[a] = hi[a];
    }
    boxes.push_back(bx);
    tri.push_back(t);
  }
};


// ------------------------------------------------------------------------------------------------
// The stages of buildBvh, in the order it runs them.
// ------------------------------------------------------------------------------------------------
struct Laps {  // BDPT_BUILD_VERBOSE: what every stage took
  const bool verbose = std::getenv("BDPT_BUILD_VERBOSE") != nullptr;
  std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
  void lap(const char* what) {
    if (!verbose) return;
    const auto t = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[bvh] %-12s %.3f s\n", what, std::chrono::duration<double>(t - last).count());
    last = t;
  }
};

// Triangle records exactly as the device intersects them — the "actual" triangle is (v0, v0+e1, v0+e2) in fp32, so
// bounds are taken from those points — and what derives from the scene's box.
struct Triangles {
  BigVec<BvhTri> recs;  // (both empty when the backend makes them where it works: `keep` = false)
  BigVec<Box> box;
  BvhSplitGrid grid;  // the scene box: the split planes are its spatial medians
  float pad;          // what every box is padded by
};
void makeTriangles(const float* positions, const uint32_t* indices, uint32_t nTris, const uint32_t* triFlags, const uint32_t* triAux, bool keep, int threads,
                   Triangles& T) {
  T.recs.resize(keep ? nTris : 0);  // (every field of every record is written by the loop below)
  T.box.resize(keep ? nTris : 0);
  Box scene;
  scene.reset();
  std::vector<Box> part((size_t)threads);
  for (Box& b : part) b.reset();
  parallelFor(nTris, threads, [&](size_t t0, size_t t1, int th) {
    Box acc;
    acc.reset();
    for (size_t t = t0; t < t1; t++) {
      const float* a = positions + (size_t)indices[t * 3] * 3;
      const float* b = positions + (size_t)indices[t * 3 + 1] * 3;
      const float* c = positions + (size_t)indices[t * 3 + 2] * 3;
      BvhTri r;
      Box bx;
      bvhTriGeom(a, b, c, r.v0, r.e1, r.e2, bx.lo, bx.hi);
      r.prim = (uint32_t)t;
      r.flags = triFlags ? triFlags[t] : 0u;
      r.aux = triAux ? triAux[t] : 0u;
      if (keep) {
        T.recs[t] = r;
        T.box[t] = bx;
      }
      acc.grow(bx);
    }
    part[(size_t)th].grow(acc);
  });
  for (const Box& b : part) scene.grow(b);
  // Slab tests run in fp32 on boxes that must never reject a hit the triangle test accepts:
  // pad every box by a small fraction of the scene diagonal, or by a few ulps of the coordinates where those are
  // larger (bvh.h bvhPadOf, which the refits share: covers rounding in both tests).
  T.pad = bvhPadOf(scene.lo, scene.hi, nTris != 0);
  for (int a = 0; a < 3; a++) {
    T.grid.lo[a] = nTris ? (double)scene.lo[a] : 0.0;
    T.grid.ext[a] = nTris ? (double)scene.hi[a] - (double)scene.lo[a] : 0.0;
  }
}

struct Budgets {
  float opaque, alpha;  // extra references per triangle of the class, on average
  float outlierArea;    // opaque triangles below this box area are never split
};
float outlierAreaOf(const Triangles& T, uint32_t nTris, float budgetOpaque) {
  if (!(budgetOpaque > 0.0f) || !nTris) return 0.0f;
  std::vector<float> areas;
  areas.reserve(nTris);
  for (uint32_t t = 0; t < nTris; t++)
    if (!(T.recs[t].flags & kTriNonOpaque)) areas.push_back(bvhBoxArea(T.box[t].lo, T.box[t].hi));  // (the area bvhRefDecide compares against it)
  if (areas.empty()) return 0.0f;
  std::nth_element(areas.begin(), areas.begin() + areas.size() / 2, areas.end());
  return (float)BDPT_SPLIT_OUTLIER * areas[areas.size() / 2];
}

// The reference decision (see "References" above): what the clipper leaves of every non-opaque triangle, every triangle's
// priority, and from those the split counts per class.
struct RefDecision {
  BigVec<uint8_t> state;  // 0 = plain reference (the triangle's box), 1 = shrunk by the clipper, 2 = dropped
  BigVec<uint32_t> splits;
  uint32_t dropped = 0;
};
constexpr size_t kRefChunk = 8192;
void decideReferences(const Triangles& T, uint32_t nTris, const BvhRefClipper* clipper, const Budgets& budgets, int threads, RefDecision& D) {
  const BigVec<BvhTri>& recs = T.recs;
  // (sized without being touched, filled side by side: 130 MB of one-thread value-initialisation at 10 M triangles otherwise)
  BigVec<double> prio(nTris);
  BigVec<float> capOf(nTris);  // splits a triangle may get at most
  BigVec<uint8_t>& state = D.state;
  BigVec<uint32_t>& splits = D.splits;
  state.resize(nTris);
  splits.resize(nTris);
  // pass 1: what the clipper leaves of every non-opaque triangle, and every triangle's priority
  parallelChunks(nTris, threads, kRefChunk, [&](size_t, size_t t0, size_t t1) {
    for (size_t t = t0; t < t1; t++) {
      auto clip = [&](double (*poly)[2], int& n) { return clipper->clip((uint32_t)t, poly, n); };
      bvhRefDecide(T.grid, recs[t], T.box[t].lo, T.box[t].hi, clipper != nullptr, clip, budgets.opaque, budgets.alpha, budgets.outlierArea, state[t], prio[t],
                   capOf[t]);
      splits[t] = 0;
    }
  });
  // split counts per class: the largest D with sum floor(D p_t) <= budget (integer sums: thread-count independent)
  for (int cls = 0; cls < 2 && nTris; cls++) {
    const float budgetF = cls ? budgets.alpha : budgets.opaque;
    if (!(budgetF > 0.0f)) continue;
    auto member = [&](size_t t) { return state[t] != 2 && (((recs[t].flags & kTriNonOpaque) != 0) == (cls == 1)); };
    uint64_t members = 0;
    double pmax = 0.0;
    {  // (a count and a maximum: what the threads find does not depend on how the range was shared out)
      std::vector<uint64_t> pm((size_t)threads, 0);
      std::vector<double> px((size_t)threads, 0.0);
      parallelFor(nTris, threads, [&](size_t t0, size_t t1, int th) {
        uint64_t m = 0;
        double x = 0.0;
        for (size_t t = t0; t < t1; t++)
          if (member(t)) {
            m++;
            x = std::max(x, prio[t]);
          }
        pm[(size_t)th] = m;
        px[(size_t)th] = x;
      });
      for (int th = 0; th < threads; th++) {
        members += pm[(size_t)th];
        pmax = std::max(pmax, px[(size_t)th]);
      }
    }
    const uint64_t budget = (uint64_t)((double)members * (double)budgetF);
    if (!members || !budget || !(pmax > 0.0)) continue;
    auto total = [&](double scale) {
      std::vector<uint64_t> part((size_t)threads, 0);
      parallelFor(nTris, threads, [&](size_t t0, size_t t1, int th) {
        uint64_t acc = 0;
        for (size_t t = t0; t < t1; t++)
          if (member(t)) acc += (uint64_t)std::min<double>(std::floor(scale * prio[t]), (double)capOf[t]);
        part[(size_t)th] = acc;
      });
      uint64_t s = 0;
      for (uint64_t v : part) s += v;
      return s;
    };
    const double scale = bvhSplitScale(pmax, budget, total);
    parallelFor(nTris, threads, [&](size_t t0, size_t t1, int) {
      for (size_t t = t0; t < t1; t++)
        if (member(t)) splits[t] = (uint32_t)std::min<double>(std::floor(scale * prio[t]), (double)capOf[t]);
    });
  }
  D.dropped = 0;
  for (uint32_t t = 0; t < nTris; t++) D.dropped += state[t] == 2 ? 1u : 0u;
}

// pass 2: the references, triangle order (chunks are contiguous triangle ranges, appended in order), as the 40-byte
// records the tree is built over (box, centre, reference index) + the triangle every reference belongs to
void makeReferences(const Triangles& T, uint32_t nTris, const BvhRefClipper* clipper, const RefDecision& D, int threads, BigVec<Ref>& refs,
                    BigVec<uint32_t>& refTri) {
  const BigVec<BvhTri>& recs = T.recs;
  const BigVec<Box>& triBox = T.box;
  std::vector<RefOut> part((nTris + kRefChunk - 1) / kRefChunk);  // one per chunk, appended in chunk order below
  parallelChunks(nTris, threads, kRefChunk, [&](size_t ci, size_t t0, size_t t1) {
    RefOut& o = part[ci];
    BigVec<BvhPiece> stack;  // the chunk's split stack: sized to a triangle's split count before it is split
    for (size_t t = t0; t < t1; t++) {
      const uint32_t splits = D.splits[t];
      if (D.state[t] == 2) continue;
      if (splits == 0 && D.state[t] == 0) {
        o.push(triBox[t].lo, triBox[t].hi, (uint32_t)t);
        continue;
      }
      // (the whole piece is recomputed here instead of kept since pass 1: a piece is ~400 bytes and a scene may hold millions)
      const bool alpha = (recs[t].flags & kTriNonOpaque) != 0 && clipper != nullptr;
      auto clip = [&](double (*poly)[2], int& n) { return clipper->clip((uint32_t)t, poly, n); };
      auto emit = [&](const BvhPiece& p) { o.push(p.lo, p.hi, (uint32_t)t); };
      BvhPiece pc;
      bool shrunk = false;
      if (!bvhWholePiece(recs[t], triBox[t].lo, triBox[t].hi, alpha, clip, pc, shrunk)) continue;  // (cannot happen: pass 1 kept it)
      if (splits == 0) {
        emit(pc);
        continue;
      }
      pc.splits = splits;
      if (stack.size() < splits) stack.resize(splits);
      bvhSplitTriangle(T.grid, recs[t], pc, alpha, stack.data(), clip, emit);
    }
  });
  std::vector<size_t> at(part.size() + 1, 0);
  for (size_t ci = 0; ci < part.size(); ci++) at[ci + 1] = at[ci] + part[ci].tri.size();
  refs.resize(at.back());
  refTri.resize(at.back());
  parallelChunks(part.size(), threads, 16, [&](size_t, size_t c0, size_t c1) {  // every chunk knows where it lands
    for (size_t ci = c0; ci < c1; ci++) {
      const RefOut& o = part[ci];
      for (size_t j = 0; j < o.tri.size(); j++) {
        Ref& r = refs[at[ci] + j];
        for (int k = 0; k < 3; k++) {  // (+ 0.0f: -0 becomes +0, so that no minimum or maximum depends on the order in which equal zeros meet)
          r.box.lo[k] = o.boxes[j].lo[k] + 0.0f;
          r.box.hi[k] = o.boxes[j].hi[k] + 0.0f;
          r.cent[k] = 0.5f * (r.box.lo[k] + r.box.hi[k]) + 0.0f;
        }
        r.id = (uint32_t)(at[ci] + j);
        refTri[at[ci] + j] = o.tri[j];
      }
      RefOut().boxes.swap(part[ci].boxes);  // (release as we go: the pieces are as large as the result)
      RefOut().tri.swap(part[ci].tri);
    }
  });
}

// The binary tree over refs[0, n), which it permutes into the leaf order.  Few references or one thread: one depth-first
// pass.  Else phase 1: one thread splits the top of the tree (large nodes share their scans among all threads) and defers
// every subtree of at most `grain` references.  Phase 2: the deferred subtrees are built concurrently, largest first,
// each into its own node list.  Phase 3: the lists are appended; children stay after parents.
void buildBinaryTree(BigVec<Ref>& refs, uint32_t n, int threads, Laps& laps, BigVec<TmpNode>& tmp) {
  BigVec<Ref> scratch(n);  // every partition scatters through the node's own range of it
  const BuildData B{refs, scratch};
  tmp.reserve((size_t)n / 2 + 16);
  tmp.push_back(makeTmpNode(0, n, 0));
  if (threads <= 1 || n < (1u << 15)) {
    buildSubtree(B, tmp, 0, 0, 1, nullptr);
    return;
  }
  const uint32_t grain = std::max<uint32_t>(4096, n / (uint32_t)(threads * 8));
  std::vector<uint32_t> deferred;
  buildSubtree(B, tmp, 0, grain, threads, &deferred);
  laps.lap("top");
  std::sort(deferred.begin(), deferred.end(), [&](uint32_t a, uint32_t b) {
    return tmp[a].count > tmp[b].count || (tmp[a].count == tmp[b].count && a < b);
  });
  std::vector<BigVec<TmpNode>> local(deferred.size());
  parallelChunks(deferred.size(), threads, 1, [&](size_t j, size_t, size_t) {
    BigVec<TmpNode>& L = local[j];
    L.reserve((size_t)tmp[deferred[j]].count / 2 + 4);
    L.push_back(tmp[deferred[j]]);
    buildSubtree(B, L, 0, 0, 1, nullptr);
  });
  laps.lap("subtrees");
  // the lists are appended in the order of `deferred` (children stay after parents); every list knows where it
  // lands, so the copies run side by side
  std::vector<size_t> at(deferred.size() + 1);
  at[0] = tmp.size();
  for (size_t j = 0; j < deferred.size(); j++) at[j + 1] = at[j] + local[j].size() - 1;
  tmp.resize(at.back());
  parallelChunks(deferred.size(), threads, 1, [&](size_t j, size_t, size_t) {
    const BigVec<TmpNode>& L = local[j];
    const int32_t off = (int32_t)at[j] - 1;  // local index i >= 1 -> off + i
    TmpNode rootNode = L[0];
    if (rootNode.left >= 0) {
      rootNode.left += off;
      rootNode.right += off;
    }
    tmp[deferred[j]] = rootNode;
    for (size_t i = 1; i < L.size(); i++) {
      TmpNode nd = L[i];
      if (nd.left >= 0) {
        nd.left += off;
        nd.right += off;
      }
      tmp[at[j] + i - 1] = nd;
    }
  });
}

// Leaf-ordered triangle list and reference boxes; `order` (a backend's tree builder left `refs` as they were): the
// reference at every position, null: `refs` are in leaf order themselves.
void gatherLeaves(const BigVec<Ref>& refs, const uint32_t* order, const BigVec<uint32_t>& refTri, const BigVec<BvhTri>& recs, int threads, Bvh& out) {
  const size_t n = refs.size();
  out.tris.resize(n);
  out.refBox.resize(n * 6);
  parallelFor(n, threads, [&](size_t a, size_t b, int) {
    for (size_t i = a; i < b; i++) {
      const Ref& r = order ? refs[order[i]] : refs[i];
      out.tris[i] = recs[refTri[r.id]];
      for (int k = 0; k < 3; k++) {
        out.refBox[i * 6 + (size_t)k] = r.box.lo[k];
        out.refBox[i * 6 + 3 + (size_t)k] = r.box.hi[k];
      }
    }
  });
}

// ---- the binary tree collapsed into four-wide nodes ----
using Wide = BvhWideNode;  // (src: tmp index of the subtree root this node covers; kids: tmp indices of the up to 4 children)
struct WideTree {
  std::vector<Wide> wide;
  std::vector<BvhSlot> slots;  // per wide node: where its index must be written
  uint32_t depth = 0, stack = 0;
};
struct Collapser {
  struct Job {
    uint32_t src, depth, stackAbove;
    int32_t slotNode, slotIdx;
  };
  const BigVec<TmpNode>& tmp;
  // Binary height of every subtree: the stack need of a subtree left two-wide is its height, so a
  // node at stack level u may widen to k children only while u + (k-1) + max child height stays
  // within the device stack.  Shallow subtrees (most of the nodes) become four-wide; only the few
  // deep, skinny paths of a SAH tree keep two-wide nodes.
  std::vector<uint16_t> height;
  std::vector<uint32_t> subtreeNodes;  // binary nodes in the subtree (itself included)
  explicit Collapser(const BigVec<TmpNode>& t) : tmp(t), height(t.size(), 0), subtreeNodes(t.size(), 1) {
    for (size_t i = tmp.size(); i-- > 0;)  // children are always created after their parent
      if (tmp[i].left >= 0) {
        height[i] = (uint16_t)(1 + std::max(height[(size_t)tmp[i].left], height[(size_t)tmp[i].right]));
        subtreeNodes[i] = 1 + subtreeNodes[(size_t)tmp[i].left] + subtreeNodes[(size_t)tmp[i].right];
      }
  }
  // One subtree, depth first, appended to W; `defer` (may be null) receives the jobs of subtrees of at most
  // kCollapseGrain binary nodes instead of descending into them.
  void run(Job rootJob, WideTree& W, std::vector<Job>* defer) const {
    std::vector<Job> jobs;
    jobs.push_back(rootJob);
    while (!jobs.empty()) {
      Job j = jobs.back();
      jobs.pop_back();
      Wide w;
      w.src = j.src;
      w.depth = j.depth;
      w.nk = 0;
      if (tmp[j.src].left < 0) {  // root is a single leaf
        w.kids[w.nk++] = j.src;
      } else {
        w.kids[w.nk++] = (uint32_t)tmp[j.src].left;
        w.kids[w.nk++] = (uint32_t)tmp[j.src].right;
        while (w.nk < 4) {
          int best = -1;
          float bestArea = -1.0f;
          for (int k = 0; k < w.nk; k++)
            if (tmp[w.kids[k]].left >= 0) {
              float ar = tmp[w.kids[k]].box.area();
              if (ar > bestArea) {
                bestArea = ar;
                best = k;
              }
            }
          if (best < 0) break;
          // stack need if we widen: j.stackAbove + nk (= (nk+1)-1) + tallest remaining child
          const uint32_t t = w.kids[best];
          uint32_t tallest = std::max<uint32_t>(height[(size_t)tmp[t].left], height[(size_t)tmp[t].right]);
          for (int k = 0; k < w.nk; k++)
            if (k != best) tallest = std::max<uint32_t>(tallest, height[w.kids[k]]);
          if (j.stackAbove + (uint32_t)w.nk + tallest > (uint32_t)kBvhMaxStack) break;
          w.kids[best] = (uint32_t)tmp[t].left;
          w.kids[w.nk++] = (uint32_t)tmp[t].right;
        }
      }
      const uint32_t self = (uint32_t)W.wide.size();
      W.wide.push_back(w);
      W.slots.push_back(BvhSlot{j.slotNode, j.slotIdx});
      W.depth = std::max(W.depth, j.depth);
      const uint32_t need = j.stackAbove + (uint32_t)(w.nk - 1);
      W.stack = std::max(W.stack, need);
      for (int k = w.nk - 1; k >= 0; k--)
        if (tmp[w.kids[k]].left >= 0) {
          const Job child{w.kids[k], j.depth + 1, need, (int32_t)self, k};
          if (defer && subtreeNodes[w.kids[k]] <= kCollapseGrain)
            defer->push_back(child);
          else
            jobs.push_back(child);
        }
    }
  }
};
// The top of the tree by one thread; the subtrees below kCollapseGrain nodes side by side, each into its own list,
// appended in the order they were met.  The grain is a constant, so the node order does not depend on the thread count.
void collapseTree(const BigVec<TmpNode>& tmp, int threads, WideTree& W) {
  using Job = Collapser::Job;
  const Collapser C(tmp);
  std::vector<Job> deferred;
  C.run(Job{0, 0, 0, -1, -1}, W, tmp.size() > 4 * (size_t)kCollapseGrain ? &deferred : nullptr);
  if (deferred.empty()) return;
  std::vector<WideTree> local(deferred.size());
  parallelChunks(deferred.size(), threads, 1, [&](size_t j, size_t, size_t) {
    WideTree& L = local[j];
    L.wide.reserve(C.subtreeNodes[deferred[j].src] / 2 + 4);
    L.slots.reserve(C.subtreeNodes[deferred[j].src] / 2 + 4);
    C.run(deferred[j], L, nullptr);  // (slots[0], a node of the top part, is a global index already)
  });
  std::vector<size_t> at(deferred.size() + 1);
  at[0] = W.wide.size();
  for (size_t j = 0; j < deferred.size(); j++) at[j + 1] = at[j] + local[j].wide.size();
  W.wide.resize(at.back());
  W.slots.resize(at.back());
  parallelChunks(deferred.size(), threads, 1, [&](size_t j, size_t, size_t) {
    const WideTree& L = local[j];
    std::copy(L.wide.begin(), L.wide.end(), W.wide.begin() + (long)at[j]);
    W.slots[at[j]] = L.slots[0];
    for (size_t i = 1; i < L.slots.size(); i++) W.slots[at[j] + i] = BvhSlot{L.slots[i].node + (int32_t)at[j], L.slots[i].idx};
  });
  for (const WideTree& L : local) {
    W.depth = std::max(W.depth, L.depth);
    W.stack = std::max(W.stack, L.stack);
  }
}

// The SAH cost: blocks of kCostBlock nodes summed in node order side by side, the block sums added in block order — the
// rounding depends on neither the thread count nor on who builds the tree.
float sahCost(const BigVec<TmpNode>& tmp, const std::vector<Wide>& wide, int threads) {
  const float rootArea = tmp[0].box.area();
  constexpr size_t kCostBlock = (size_t)1 << 16;
  std::vector<double> part((wide.size() + kCostBlock - 1) / kCostBlock, 0.0);
  if (rootArea > 0)
    parallelChunks(wide.size(), threads, kCostBlock, [&](size_t ci, size_t w0, size_t w1) {
      double cost = 0.0;
      for (size_t wi = w0; wi < w1; wi++)
        for (int k = 0; k < wide[wi].nk; k++) {
          const TmpNode& c = tmp[wide[wi].kids[k]];
          cost += (c.left < 0 ? kCostTri * c.count : kCostTraverse) * c.box.area() / rootArea;
        }
      part[ci] = cost;
    });
  double cost = 0.0;
  for (double v : part) cost += v;
  return (float)cost + kCostTraverse;
}

// Child boxes padded, then quantised (bvh.h bvhQuantiseNode: the device build and the refits run the same code).
void quantiseNodes(const BigVec<TmpNode>& tmp, const WideTree& W, float pad, int threads, BigVec<BvhNode>& nodes) {
  nodes.resize(W.wide.size());
  parallelFor(W.wide.size(), threads, [&](size_t w0, size_t w1, int) {
    for (size_t wi = w0; wi < w1; wi++) {
      const Wide& w = W.wide[wi];
      BvhNode nd;
      std::memset(&nd, 0, sizeof(nd));
      float clo[4][3], chi[4][3];
      for (int k = 0; k < w.nk; k++)
        for (int a = 0; a < 3; a++) {
          clo[k][a] = tmp[w.kids[k]].box.lo[a] - pad;
          chi[k][a] = tmp[w.kids[k]].box.hi[a] + pad;
        }
      uint32_t q[10];
      bvhQuantiseNode(clo, chi, w.nk, q);
      std::memcpy(nd.origin, &q[0], 12);
      for (int a = 0; a < 3; a++) {
        const uint32_t sb = ((q[3] >> (8 * a)) & 0xffu) << 23;
        std::memcpy(&nd.scale[a], &sb, 4);
      }
      std::memcpy(nd.lo, &q[4], 12);
      std::memcpy(nd.hi, &q[7], 12);
      for (int k = 0; k < 4; k++) nd.child[k] = -1;
      for (int k = 0; k < w.nk; k++) {
        const TmpNode& c = tmp[w.kids[k]];
        if (c.left < 0) nd.child[k] = -1 - (int32_t)((c.first << 3) | (c.count - 1));  // leaf reference; interior ones are patched below
      }
      nodes[wi] = nd;
    }
  });
  for (size_t wi = 1; wi < W.wide.size(); wi++) nodes[(size_t)W.slots[wi].node].child[W.slots[wi].idx] = (int32_t)wi;
}

// Nothing to build a tree over: one node without children.
void emptyTree(Bvh& out) {
  BvhNode nd;
  std::memset(&nd, 0, sizeof(nd));
  for (int a = 0; a < 3; a++)
    for (int c = 0; c < 4; c++) {
      nd.lo[a][c] = 255;
      nd.hi[a][c] = 0;
    }
  for (int c = 0; c < 4; c++) nd.child[c] = -1;
  nd.scale[0] = nd.scale[1] = nd.scale[2] = 1.0f;
  out.nodes.push_back(nd);
  out.numNodes = 1;
  packBvh(out, 1);
}

float budgetOr(float asked, const char* env, float dflt) {
  if (asked >= 0.0f) return asked;
  if (const char* e = std::getenv(env)) {
    const float v = (float)std::atof(e);
    if (v >= 0.0f && v <= 64.0f) return v;
  }
  return dflt;
}

BvhBackend gDefaultBackend;

}  // namespace

void bvhSetDefaultBackend(const BvhBackend& b) { gDefaultBackend = b; }

int bvhBuildThreads() {
  if (const char* e = std::getenv("BDPT_BUILD_THREADS")) {
    const int v = std::atoi(e);
    if (v >= 1) return std::min(v, 256);
  }
  int n = (int)std::thread::hardware_concurrency();
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof(set), &set) == 0) n = std::min(n > 0 ? n : 1 << 20, CPU_COUNT(&set));
  if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {  // container CPU quota: "<quota> <period>" or "max <period>"
    char q[64];
    double period = 0;
    if (std::fscanf(f, "%63s %lf", q, &period) == 2 && std::strcmp(q, "max") != 0 && period > 0)
      n = std::min(n, std::max(1, (int)(std::atof(q) / period + 0.5)));
    std::fclose(f);
  }
  return std::max(1, std::min(n, 64));
}

void buildBvh(const float* positions, const uint32_t* indices, uint32_t n, const uint32_t* triFlags, Bvh& out, int threads,
              const uint32_t* triAux) {
  BvhBuildOptions opt;
  opt.threads = threads;
  buildBvh(positions, indices, n, triFlags, out, opt, triAux);
}

void buildBvh(const float* positions, const uint32_t* indices, uint32_t nTris, const uint32_t* triFlags, Bvh& out,
              const BvhBuildOptions& opt, const uint32_t* triAux) {
  const int threads = opt.threads > 0 ? opt.threads : bvhBuildThreads();
  Laps laps;
  out = Bvh();
  auto fail = [&](const std::string& err, const char* what) {
    if (opt.error) *opt.error = err.empty() ? what : err;
  };
  // where the stages run: all here, the binary tree alone on the backend, or references, tree and everything after it
  const BvhBackend be = opt.backend ? *opt.backend : gDefaultBackend;
  const bool whole = be.makeRefs && be.buildTree && be.pack;
  if (!whole && (be.makeRefs || be.pack)) return fail("", "build backend: a reference maker and a packer need each other and a tree builder");
  Budgets budgets;
  budgets.opaque = budgetOr(opt.splitBudget, "BDPT_SPLIT_BUDGET", (float)BDPT_SPLIT_BUDGET);
  budgets.alpha = budgetOr(opt.splitBudgetAlpha, "BDPT_SPLIT_BUDGET_ALPHA", (float)BDPT_SPLIT_BUDGET_ALPHA);
  // the backend does all of the reference stage, pass 1 and the split counts included ...
  const bool decideThere = whole && !be.hostPriorities;
  // ... and then makes the triangle records and their boxes where it works, from positions + indices: this side only
  // needs the scene's box, not 72 bytes per triangle written and page-faulted in (0.05-0.15 s of a 10 M-triangle bdpt_set_scene)
  const bool recsThere = decideThere && !be.uploadTriRecs && opt.numVertices != 0 && !(budgets.opaque > 0.0f);

  Triangles T;
  makeTriangles(positions, indices, nTris, triFlags, triAux, !recsThere, threads, T);
  budgets.outlierArea = outlierAreaOf(T, nTris, budgets.opaque);
  RefDecision D;
  if (!decideThere) decideReferences(T, nTris, opt.clipper, budgets, threads, D);
  laps.lap("priorities");

  BigVec<Ref> refs;  // (stay empty when the backend makes them: it keeps them for its tree builder and its packer)
  BigVec<uint32_t> refTri;
  uint32_t n = 0;  // references from here on
  std::string err;
  if (whole) {
    BvhRefInput in{};
    in.triRecs = recsThere ? nullptr : T.recs.data();
    in.triBox = recsThere ? nullptr : T.box.data();
    in.uploadTriRecs = be.uploadTriRecs || opt.numVertices == 0;
    in.splits = decideThere ? nullptr : D.splits.data();
    in.state = decideThere ? nullptr : D.state.data();
    in.numTris = nTris;
    in.budgetOpaque = budgets.opaque;
    in.budgetAlpha = budgets.alpha;
    in.outlierArea = budgets.outlierArea;
    in.numDroppedOut = decideThere ? &D.dropped : nullptr;
    for (int a = 0; a < 3; a++) {
      in.gridLo[a] = T.grid.lo[a];
      in.gridExt[a] = T.grid.ext[a];
    }
    in.clipper = opt.clipper;
    in.positions = positions;
    in.indices = indices;
    in.triFlags = triFlags;
    in.triAux = triAux;
    in.numVertices = opt.numVertices;
    if (!be.makeRefs(be.user, in, n, err)) return fail(err, "reference maker failed");
  } else {
    makeReferences(T, nTris, opt.clipper, D, threads, refs, refTri);
    n = (uint32_t)refs.size();
  }
  out.numDropped = D.dropped;
  out.numRefs = n;
  if (laps.verbose) std::fprintf(stderr, "[bvh] %u triangles -> %u references (%u dropped)\n", nTris, n, out.numDropped);
  laps.lap("records");

  // the binary tree: on the backend the same decisions, the same order of the references, the same tree as the host code
  BigVec<TmpNode> tmp;
  BigVec<uint32_t> order;  // filled by a backend's tree builder that was handed `refs`: the leaf order as reference ids (the host code permutes `refs` itself)
  const bool treeThere = be.buildTree && n > 0;
  if (treeThere) {
    if (!be.buildTree(be.user, whole ? nullptr : refs.data(), n, order, tmp, err) || tmp.empty() || (!whole && order.size() != n))
      return fail(err, "tree builder failed");
    laps.lap("device tree");
  } else {
    buildBinaryTree(refs, n, threads, laps, tmp);
  }
  laps.lap("append");

  if (whole && treeThere) {
    // collapse, quantisation, packing, the summary: where the tree is
    const BvhPackInput in{nTris, n, T.pad};
    if (!be.pack(be.user, in, out, err)) {
      fail(err, "packer failed");
      out.deviceRecs = nullptr;
      out.deviceNumRecs = 0;
    }
    laps.lap("device collapse + pack");
    return;
  }
  if (n == 0) return emptyTree(out);
  gatherLeaves(refs, treeThere ? order.data() : nullptr, refTri, T.recs, threads, out);
  WideTree W;
  collapseTree(tmp, threads, W);
  laps.lap("collapse");
  out.maxDepth = W.depth;
  out.maxStack = W.stack;
  out.numNodes = (uint32_t)W.wide.size();
  quantiseNodes(tmp, W, T.pad, threads, out.nodes);
  out.sahCost = sahCost(tmp, W.wide, threads);
  laps.lap("quantise");
  if (!packBvh(out, threads)) out.recs.clear();  // (leaves of at most 8 triangles always fit: 3 x 8 < 256)
  laps.lap("pack");
}

bool packBvh(Bvh& bvh, int threads) {
  if (threads <= 0) threads = bvhBuildThreads();
  const size_t nn = bvh.nodes.size();
  // record index of every node, and of every node's first child: parents come before their children in `nodes`,
  // so one pass in index order hands out the child blocks (a node's block follows the blocks of all earlier nodes)
  std::vector<uint32_t> pos(nn, 0), base(nn, 0);
  uint64_t next = 1;  // record 0 = the root
  for (size_t i = 0; i < nn; i++) {
    const BvhNode& n = bvh.nodes[i];
    const int nk = bvhNumChildren(n);
    base[i] = (uint32_t)next;
    for (int c = 0; c < nk; c++) {
      const int32_t r = n.child[c];
      if (r >= 0) {
        if ((size_t)r <= i || (size_t)r >= nn) return false;
        pos[(size_t)r] = (uint32_t)next;
        next += 1;
      } else {
        next += (uint64_t)(((uint32_t)(-1 - r)) & 7u) + 1u;
      }
    }
    if (next >= 0x7fffffffull) return false;
  }
  // every record below `next` is written by the loop below (a node at pos[i], a leaf's triangles behind base[i]); the pad
  // records behind them — the device fetches up to four records per leaf visit — are zero
  bvh.recs.resize((size_t)next + kBvhPadRecs);
  for (uint32_t k = 0; k < kBvhPadRecs; k++) bvh.recs[(size_t)next + k] = BvhRec{};
  bool ok = true;
  std::mutex failMutex;
  parallelFor(nn, threads, [&](size_t i0, size_t i1, int) {
    for (size_t i = i0; i < i1; i++) {
      const BvhNode& n = bvh.nodes[i];
      BvhRec rec{};
      std::memcpy(&rec.w[0], n.origin, 12);
      uint32_t ex[3];
      for (int a = 0; a < 3; a++) {
        uint32_t bits;
        std::memcpy(&bits, &n.scale[a], 4);
        ex[a] = (bits >> 23) & 0xffu;  // the scales are powers of two: mantissa 0, sign 0
      }
      std::memcpy(&rec.w[4], n.lo, 12);
      std::memcpy(&rec.w[7], n.hi, 12);
      const int nk = bvhNumChildren(n);
      uint32_t leafBits = 0, offs = 0, off = 0;
      for (int c = 0; c < nk; c++) {
        if (off > 255u) {
          std::lock_guard<std::mutex> g(failMutex);
          ok = false;
          break;
        }
        offs |= off << (8 * c);
        const int32_t r = n.child[c];
        if (r >= 0) {
          off += 1;
        } else {
          leafBits |= 1u << c;
          const uint32_t enc = (uint32_t)(-1 - r), first = enc >> 3, cnt = (enc & 7u) + 1u;
          for (uint32_t k = 0; k < cnt; k++) {
            BvhTri t = bvh.tris[first + k];
            if (k + 1 == cnt) t.flags |= kTriLastOfLeaf;
            std::memcpy(&bvh.recs[(size_t)base[i] + off + k], &t, sizeof(BvhTri));
          }
          off += cnt;
        }
      }
      rec.w[3] = ex[0] | (ex[1] << 8) | (ex[2] << 16) | (leafBits << 24);
      rec.w[10] = base[i];
      rec.w[11] = offs;
      bvh.recs[pos[i]] = rec;
    }
  });
  return ok;
}

// ------------------------------------------------------------------------------------------------
// Refit (bvh.h "refit"): the plan from the records, the host refit, the SAH of a refitted tree.
// ------------------------------------------------------------------------------------------------
// children of a packed node: slots up to the last one whose box is not the unused slot's (lo = 255, hi = 0 on every
// axis), as bvhNumChildren counts them on a BvhNode
static uint32_t recNumChildren(const BvhRec& n) {
  uint32_t nk = 0;
  for (uint32_t c = 0; c < 4; c++) {
    bool empty = true;
    for (int a = 0; a < 3; a++)
      if (((n.w[4 + a] >> (8 * c)) & 0xffu) != 255u || ((n.w[7 + a] >> (8 * c)) & 0xffu) != 0u) empty = false;
    if (!empty) nk = c + 1;
  }
  return nk;
}

bool bvhRefitMakePlan(const BvhRec* recs, size_t numRecs, BvhRefitPlan& plan, std::string& err) {
  plan.nodes.clear();
  plan.levelOrder.clear();
  plan.levelStart.clear();
  if (numRecs <= kBvhPadRecs) {
    err = "refit: no records";
    return false;
  }
  const size_t used = numRecs - kBvhPadRecs;
  // top-down, level by level: the interior records of every depth
  std::vector<std::vector<uint32_t>> levels(1, std::vector<uint32_t>(1, 0u));
  std::vector<uint8_t> seen(used, 0);
  seen[0] = 1;
  for (size_t l = 0; l < levels.size(); l++) {
    std::vector<uint32_t> next;
    for (uint32_t r : levels[l]) {
      const BvhRec& n = recs[r];
      const int nk = (int)recNumChildren(n);
      for (int c = 0; c < nk; c++) {
        const uint64_t at = (uint64_t)n.w[10] + ((n.w[11] >> (8 * c)) & 0xffu);
        if (at >= used) {
          err = "refit: a child lies outside the record array";
          return false;
        }
        if ((n.w[3] >> (24 + c)) & 1u) continue;  // leaf: its triangles are counted below
        if (seen[at]) {
          err = "refit: a record is reached twice";
          return false;
        }
        seen[at] = 1;
        next.push_back((uint32_t)at);
      }
    }
    if (!next.empty()) {
      if (levels.size() > 64) {
        err = "refit: the tree is deeper than 64 levels";
        return false;
      }
      levels.push_back(std::move(next));
    }
  }
  // build order: childBase ascending (packBvh / bvh_device.hip k_write_recs hand the child blocks out in node order)
  std::vector<std::pair<uint32_t, uint32_t>> byBase;  // (childBase, record)
  std::vector<uint32_t> depthOf;
  for (size_t l = 0; l < levels.size(); l++)
    for (uint32_t r : levels[l]) byBase.emplace_back(recs[r].w[10], r);
  std::sort(byBase.begin(), byBase.end());
  std::vector<uint32_t> nodeOfRec(used, 0xffffffffu);
  for (size_t i = 0; i < byBase.size(); i++) nodeOfRec[byBase[i].second] = (uint32_t)i;
  plan.nodes.resize(byBase.size());
  for (size_t i = 0; i < byBase.size(); i++) {
    const uint32_t r = byBase[i].second;
    const BvhRec& n = recs[r];
    BvhRefitNode& nd = plan.nodes[i];
    nd.rec = r;
    nd.nk = recNumChildren(n);
    for (int c = 0; c < 4; c++) nd.kid[c] = 0;
    for (uint32_t c = 0; c < nd.nk; c++) {
      const size_t at = (size_t)n.w[10] + ((n.w[11] >> (8 * c)) & 0xffu);
      if (!((n.w[3] >> (24 + c)) & 1u)) {
        nd.kid[c] = nodeOfRec[at];
        continue;
      }
      uint32_t cnt = 0;
      for (;;) {  // a leaf's triangles end at the one flagged kTriLastOfLeaf; at most 8
        if (at + cnt >= used || cnt >= 8 || nodeOfRec[at + cnt] != 0xffffffffu || seen[at + cnt]) {
          err = "refit: a leaf's triangles are not where its parent says";
          return false;
        }
        seen[at + cnt] = 1;
        const bool last = (recs[at + cnt].w[7] & kTriLastOfLeaf) != 0;
        cnt++;
        if (last) break;
      }
      nd.kid[c] = kRefitLeaf | cnt;
    }
  }
  for (size_t l = levels.size(); l-- > 0;) {
    plan.levelStart.push_back((uint32_t)plan.levelOrder.size());
    for (uint32_t r : levels[l]) plan.levelOrder.push_back(nodeOfRec[r]);
  }
  plan.levelStart.push_back((uint32_t)plan.levelOrder.size());
  return true;
}

float bvhRefitSah(const BvhRefitPlan& plan, const float* rootBox, const float* childArea) {
  const float rootArea = bvhBoxArea(rootBox, rootBox + 3);
  constexpr size_t kCostBlock = (size_t)1 << 16;
  double cost = 0.0;
  if (rootArea > 0)
    for (size_t b0 = 0; b0 < plan.nodes.size(); b0 += kCostBlock) {
      double part = 0.0;
      const size_t b1 = std::min(plan.nodes.size(), b0 + kCostBlock);
      for (size_t wi = b0; wi < b1; wi++)
        for (uint32_t k = 0; k < plan.nodes[wi].nk; k++) {
          const uint32_t kd = plan.nodes[wi].kid[k];
          part += (kd & kRefitLeaf ? kCostTri * (float)(kd & ~kRefitLeaf) : kCostTraverse) * childArea[wi * 4 + k] / rootArea;
        }
      cost += part;
    }
  return (float)cost + kCostTraverse;
}

void bvhPieceRegionsHost(const BvhRec* recs, size_t numRecs, const BvhRefitPlan& plan, std::vector<float>& region, int threads) {
  if (threads <= 0) threads = bvhBuildThreads();
  region.assign(numRecs * kPieceFloats, 0.0f);
  parallelFor(plan.nodes.size(), threads, [&](size_t i0, size_t i1, int) {
    for (size_t i = i0; i < i1; i++) bvhPieceRegionsOfNode(plan.nodes[i], recs, region.data());
  });
}

void bvhRefitHost(BvhRec* recs, const BvhRefitPlan& plan, const float* positions, const uint32_t* indices, uint32_t numTris,
                  std::vector<float>& box, std::vector<float>& childArea, int threads, const float* pieces) {
  if (threads <= 0) threads = bvhBuildThreads();
  float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};  // the scene box over every input triangle
  for (uint32_t t = 0; t < numTris; t++) {
    float v0[3], e1[3], e2[3], tl[3], th[3];
    bvhTriGeom(positions + (size_t)indices[(size_t)t * 3] * 3, positions + (size_t)indices[(size_t)t * 3 + 1] * 3,
               positions + (size_t)indices[(size_t)t * 3 + 2] * 3, v0, e1, e2, tl, th);
    for (int a = 0; a < 3; a++) {
      lo[a] = tl[a] < lo[a] ? tl[a] : lo[a];
      hi[a] = hi[a] < th[a] ? th[a] : hi[a];
    }
  }
  const float pad = bvhPadOf(lo, hi, numTris != 0);
  box.assign(plan.nodes.size() * 6, 0.0f);
  childArea.assign(plan.nodes.size() * 4, 0.0f);
  for (size_t l = 0; l + 1 < plan.levelStart.size(); l++) {
    const size_t a = plan.levelStart[l], n = plan.levelStart[l + 1] - a;
    parallelFor(n, threads, [&](size_t i0, size_t i1, int) {
      for (size_t i = i0; i < i1; i++) {
        const uint32_t self = plan.levelOrder[a + i];
        if (pieces)
          bvhRefitNodePieces(plan.nodes[self], self, recs, positions, indices, box.data(), childArea.data(), pad, pieces);
        else
          bvhRefitNode(plan.nodes[self], self, recs, positions, indices, box.data(), childArea.data(), pad);
      }
    });
  }
}

}  // namespace bdpt
