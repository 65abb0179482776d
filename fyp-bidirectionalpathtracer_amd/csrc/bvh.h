// bvh.h — host-side acceleration-structure build.  Replaces the DXR driver's
// BuildRaytracingAccelerationStructure calls issued by Falcor
// (Raytracing/RtModel.cpp:181-254 bottom level, Raytracing/RtScene.cpp:220-308 top level);
// instancing is flattened on input so one level suffices.
#pragma once
#include <cstdint>
#include <vector>

#include <math.h>
#include <cstdlib>
#include <exception>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

namespace bdpt {
// std::vector whose resize() leaves new elements UNINITIALISED (default-initialisation instead of value-initialisation):
// the builder's arrays are hundreds of megabytes each and are filled by parallel loops right after they are sized;
// letting one thread zero them first — and take every page fault — cost more than the loops (round 4: 8 GB of such
// fills in a 10 M-triangle build).  Only for element types whose default-initialisation does nothing, and only where
// every element is written before it is read.
template <class T>
struct NoInitAllocator : std::allocator<T> {
  template <class U>
  struct rebind {
    using other = NoInitAllocator<U>;
  };
  NoInitAllocator() = default;
  template <class U>
  NoInitAllocator(const NoInitAllocator<U>&) {}
  template <class U>
  void construct(U* p) {
    ::new (static_cast<void*>(p)) U;
  }
  template <class U, class A0, class... A>
  void construct(U* p, A0&& a0, A&&... a) {
    ::new (static_cast<void*>(p)) U(static_cast<A0&&>(a0), static_cast<A&&>(a)...);
  }
};
template <class T>
using BigVec = std::vector<T, NoInitAllocator<T>>;

// Worker threads of the host-side builder.  An exception thrown on a worker (std::bad_alloc from the large per-chunk
// allocations of a 10 M-triangle scene, above all) must not reach std::terminate: it is kept, every thread is joined,
// and join() rethrows it on the caller's thread, where bdpt_set_scene turns it into BDPT_E_NOMEM.  Leaving the scope
// early (the caller's own chunk threw) joins the threads as well.
class WorkerScope {
 public:
  template <class F>
  void spawn(F f) {
    mPool.emplace_back([this, f] {
      try {
        if (std::getenv("BDPT_TEST_THROW_IN_WORKER")) throw std::bad_alloc();  // test hook: tests/test_bvh_builder.py
        f();
      } catch (...) {
        std::lock_guard<std::mutex> g(mLock);
        if (!mError) mError = std::current_exception();
      }
    });
  }
  void join() {
    for (std::thread& t : mPool) t.join();
    mPool.clear();
    if (mError) {
      std::exception_ptr e = mError;
      mError = nullptr;
      std::rethrow_exception(e);
    }
  }
  ~WorkerScope() {
    for (std::thread& t : mPool)
      if (t.joinable()) t.join();
  }

 private:
  std::vector<std::thread> mPool;
  std::exception_ptr mError;
  std::mutex mLock;
};


// 64-byte four-child node with child boxes quantised to 8 bits per plane relative to the node's
// own box: plane = origin[axis] + q * scale[axis], scale a power of two.  Quantisation rounds outward, so a
// decoded child box always contains the (already padded) exact one.  One node = four 16-byte
// loads per lane, the same as a two-child fp32 node, for half the dependent fetches per ray.
//   ref >= 0 : interior node index
//   ref <  0 : leaf, -1 - ((firstTriangle << 3) | (count - 1)), count in 1..8
// Unused child slots have lo = 255, hi = 0 on every axis (never entered: the slab test picks
// near/far planes by ray direction sign, so an inverted box has tnear > tfar).
// (The scales are stored as ready-to-use floats, not as exponent bytes: the node visit is bound by VALU issue and the
// decode cost six instructions per visit; the child count is implied by the inverted boxes of unused slots.)
struct alignas(16) BvhNode {
  float origin[3];
  float scale[3];    // 2^e per axis
  uint8_t lo[3][4];  // [axis][child]
  uint8_t hi[3][4];
  int32_t child[4];
};
inline int bvhNumChildren(const BvhNode& n) {
  int k = 0;
  for (int c = 0; c < 4; c++)
    if (!(n.lo[0][c] == 255 && n.hi[0][c] == 0 && n.lo[1][c] == 255 && n.hi[1][c] == 0 && n.lo[2][c] == 255 && n.hi[2][c] == 0)) k = c + 1;
  return k;
}
static_assert(sizeof(BvhNode) == 64, "node must be 64 bytes");

// 48-byte leaf triangle as intersected: v0, e1 = v1 - v0, e2 = v2 - v0 (+ ids in the w lanes).
struct alignas(16) BvhTri {
  float v0[3];
  uint32_t prim;  // index into the caller's triangle list
  float e1[3];
  uint32_t flags;  // bit0 non-opaque (any-hit alpha test), bit1 double-sided (no back-face cull)
  float e2[3];
  uint32_t aux;  // caller's word per triangle (bdpt_set_scene: index of the alpha-test record of a non-opaque triangle)
};
static_assert(sizeof(BvhTri) == 48, "triangle must be 48 bytes");

#ifndef KSTACK
#define KSTACK 32
#endif
#ifndef BDPT_BVH_STACK_BUDGET
#define BDPT_BVH_STACK_BUDGET (KSTACK - 1)
#endif
constexpr int kBvhMaxStack = BDPT_BVH_STACK_BUDGET;  // worst-case traversal stack entries (the device stack holds KSTACK per lane)
constexpr uint32_t kTriNonOpaque = 1u, kTriDoubleSided = 2u;

// What the device traverses: ONE array of 48-byte records in which a node's children — interior nodes (one record
// each) and leaves (their triangles, one BvhTri record each) — follow one another from `childBase` on.
// A divergent wave pays for every 16-byte load of every lane (the vector-memory address unit takes one lane-load per
// clock per CU: profiles/README.md), so a node visit is three loads here instead of four:
//   word 0-2  origin.xyz (float)
//   word 3    biased scale exponents ex | ey << 8 | ez << 16 (scale = 2^(e-127)), leaf bits << 24 (bit c: child c is a leaf)
//   word 4-9  lo.x lo.y lo.z hi.x hi.y hi.z, four child bytes each (as BvhNode)
//   word 10   childBase: record index of the first child
//   word 11   record offset of child c from childBase in byte c (child 0: 0)
// Device references: ref >= 0 interior record index; ref < 0 leaf, ~ref = record index of its first triangle; the last
// triangle of a leaf carries kTriLastOfLeaf in its flags.  The root is record 0; kBvhPadRecs zero pad records end the array.
constexpr int kRecF4 = 3;  // 16-byte words per record
struct alignas(16) BvhRec {
  uint32_t w[4 * kRecF4];
};
static_assert(sizeof(BvhRec) == 48, "record size");
constexpr uint32_t kTriLastOfLeaf = 4u;  // BvhTri::flags bit set by packBvh (device-side records only)
constexpr uint32_t kBvhPadRecs = 4;      // zero records behind the array (a leaf fetch reads past a leaf's last triangle)

struct Bvh {
  BigVec<BvhNode> nodes;
  BigVec<BvhTri> tris;   // in leaf order: one record per REFERENCE (a split triangle appears once per piece)
  BigVec<float> refBox;  // 6 floats (lo, hi) per entry of `tris`: bounds of the piece the reference stands for
  BigVec<BvhRec> recs;   // packed device form of the two (packBvh)
  uint32_t maxDepth = 0;     // depth of the four-wide tree
  uint32_t maxStack = 0;     // worst-case number of simultaneously stacked references
  float sahCost = 0.0f;
  uint32_t numDropped = 0;   // input triangles with no reference at all (the clipper found nothing that can be hit)
  uint32_t numNodes = 0;     // four-wide nodes and references (= nodes.size(), tris.size() when the host code packed)
  uint32_t numRefs = 0;
  // With BvhBackend::pack: the packed records are built in device memory and nodes / tris / refBox / recs stay empty.
  void* deviceRecs = nullptr;  // hipMalloc'ed, the caller's to free
  size_t deviceNumRecs = 0;    // (including the kBvhPadRecs pad records)
};

// Lets the caller shrink or drop the part of a triangle a reference stands for.  Used for non-opaque triangles
// (flag kTriNonOpaque): a hit is only ever reported where the any-hit alpha test passes, so a piece whose texels
// all fail can never produce a hit and needs no reference, and a reference only has to bound the part of its
// piece where the test can pass.  `poly` is a convex polygon in the triangle's barycentric plane, vertex k =
// (bu, bv) with P = v0 + bu e1 + bv e2, at most kBvhPolyMax vertices.  Returns false when nothing is left.
constexpr int kBvhPolyMax = 24;
// Opaque triangles are only split when their box is an outlier — at least BDPT_SPLIT_OUTLIER times the median box area of
// the scene's opaque triangles — and only down to about that size (bvh_build.cpp "References"); no triangle is split more
// than BDPT_SPLIT_MAX_PER_TRI times.
#ifndef BDPT_SPLIT_OUTLIER
#define BDPT_SPLIT_OUTLIER 8.0f
#endif
#ifndef BDPT_SPLIT_MAX_PER_TRI
#define BDPT_SPLIT_MAX_PER_TRI 255
#endif
#ifdef __HIPCC__
#define BVH_HD __host__ __device__
#else
#define BVH_HD
#endif
// Cube root of a non-negative finite double in plain arithmetic — exponent reduced to a multiple of three by bit
// manipulation, six Newton steps on the mantissa — so that the host compiler and the device compiler produce the same bits
// (libm's cbrt is correctly rounded on neither in general, and the two differ): the split priorities are computed with it.
BVH_HD inline double bvhCbrt(double x) {
  if (!(x > 0.0)) return 0.0;
  int scaled = 0;
  if (x < 2.2250738585072014e-308) {  // denormal: an exact scaling by 2^108 first, 2^-36 at the end
    x *= 324518553658426726783156020576256.0;
    scaled = -36;
  }
  unsigned long long u;
  __builtin_memcpy(&u, &x, 8);
  const int e = (int)((u >> 52) & 0x7ffull) - 1023;
  const int q = e >= 0 ? e / 3 : -((-e + 2) / 3);
  const int r = e - 3 * q;  // 0, 1, 2
  u = (u & 0x000fffffffffffffull) | ((unsigned long long)(1023 + r) << 52);
  double m;
  __builtin_memcpy(&m, &u, 8);  // in [1, 8)
  double t = m < 2.0 ? 1.1 : (m < 4.0 ? 1.4 : 1.8);
  for (int i = 0; i < 6; i++) t = t - (t * t * t - m) / (3.0 * t * t);
  const unsigned long long p = (unsigned long long)(1023 + q + scaled) << 52;
  double s2;
  __builtin_memcpy(&s2, &p, 8);
  return t * s2;
}
// What a clipper decides with, as plain tables — for the same decisions somewhere else (the device: bvh_device.hip runs
// bvh_refs.h's bvhClipPoly, the text of alpha_clip.cpp's clip(), on copies of these).  All pointers stay the clipper's /
// the scene's.
struct BvhClipTables {
  const uint32_t* triMaterial = nullptr;  // per triangle
  const uint32_t* indices = nullptr;      // 3 per triangle
  const float* texcoords = nullptr;       // 3 floats per vertex, or null
  uint32_t numTriangles = 0, numVertices = 0;
  std::vector<int32_t> matMask;     // per material: index into masks, -1: no texture decides
  std::vector<int32_t> matVerdict;  // for matMask < 0: 1 the test always passes, 2 it always fails
  struct Mask {
    int32_t w, h;
    const uint32_t* mayPass;  // summed-area table, (w + 1) x (h + 1): cells a sample may pass in
  };
  std::vector<Mask> masks;
};
struct BvhRefClipper {
  virtual ~BvhRefClipper() {}
  virtual bool clip(uint32_t tri, double (*poly)[2], int& n) const = 0;
  virtual bool tables(BvhClipTables&) const { return false; }  // false: this clipper's decisions exist as code only
};

// ---- what the binary-tree stage of the builder works on (bvh_build.cpp on the host, bvh_device.hip on the device) ----
#ifndef BDPT_SAH_BINS
#define BDPT_SAH_BINS 16
#endif
#ifndef BDPT_LEAF_MAX
#define BDPT_LEAF_MAX 2
#endif
constexpr int kBvhBins = BDPT_SAH_BINS;           // SAH bins per axis
constexpr uint32_t kBvhLeafMax = BDPT_LEAF_MAX;   // references per leaf, at most 8 (three count bits in a leaf reference)
constexpr int kBvhBinaryMaxDepth = kBvhMaxStack;  // depth budget of the binary tree: a two-wide path stacks one reference per level
struct BvhBox {
  float lo[3], hi[3];
  void reset() {
    lo[0] = lo[1] = lo[2] = 1e30f;
    hi[0] = hi[1] = hi[2] = -1e30f;
  }
  void grow(const BvhBox& b) {
    for (int a = 0; a < 3; a++) {
      lo[a] = b.lo[a] < lo[a] ? b.lo[a] : lo[a];  // std::min(lo, b.lo)
      hi[a] = hi[a] < b.hi[a] ? b.hi[a] : hi[a];  // std::max(hi, b.hi)
    }
  }
  void grow(const float* p) {
    for (int a = 0; a < 3; a++) {
      lo[a] = p[a] < lo[a] ? p[a] : lo[a];
      hi[a] = hi[a] < p[a] ? p[a] : hi[a];
    }
  }
  float area() const {
    float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    if (dx < 0 || dy < 0 || dz < 0) return 0.0f;
    return 2.0f * (dx * dy + dy * dz + dz * dx);
  }
};
// One reference: the box of the piece it stands for, the box's centre, its index in the reference list.  The
// records themselves are permuted as nodes are partitioned; a node owns a contiguous range.
struct BvhBuildRef {
  BvhBox box;
  float cent[3];
  uint32_t id;
};
static_assert(sizeof(BvhBuildRef) == 40, "reference record");
struct BvhBuildNode {  // (no member initialisers: arrays of these are sized without being touched)
  BvhBox box;
  int32_t left, right;    // children (indices into the node list, always behind their parent) or -1
  uint32_t first, count;  // leaf: its range of the reference array
  uint32_t depth;
};
static_assert(sizeof(BvhBuildNode) == 44, "binary node");
// ---- the stages of buildBvh that can run somewhere else (bdpt_set_scene: on the device, bvh_device.hip) ----
// Each produces what the host code of bvh_build.cpp produces, bit for bit, and hands it to the next one of the same `user`
// where it works.  false + err on failure.
//
// Makes the references (bvh_build.cpp "References": every triangle's whole piece, shrunk by the clipper, split `splits`
// times, every piece clipped again) in the host code's order and keeps them, the triangle of each and the triangle
// records for the two stages below.
struct BvhRefInput {
  const BvhTri* triRecs;   // one per input triangle; null with triBox: made from positions / indices / triFlags / triAux
  const BvhBox* triBox;    // where the maker works (buildBvh "Triangle records": plain fp32 arithmetic, bit-identical)
  bool uploadTriRecs;      // the two arrays above are there and are the ones to use
  const uint32_t* splits;  // split count per triangle; null: the maker also decides what the clipper leaves of every
  const uint8_t* state;    // triangle (state: 0 = plain reference (triBox), 1 = shrunk by the clipper, 2 = dropped), its split
  uint32_t numTris;        // priority and the split counts that meet the budgets below (bvh_build.cpp pass 1 + "split counts")
  float budgetOpaque, budgetAlpha;  // extra references per triangle of the class, on average (0: the class is not split)
  float outlierArea;                // opaque triangles below this box area are never split
  uint32_t* numDroppedOut;          // (with splits == null) receives the number of dropped triangles
  double gridLo[3], gridExt[3];      // the scene box: the split planes are its spatial medians
  const BvhRefClipper* clipper;      // for the non-opaque triangles; may be null
  const float* positions;            // buildBvh's inputs: (12 numVertices + 20 numTris) bytes to hand over instead of
  const uint32_t* indices;           // the 72 numTris of triRecs + triBox
  const uint32_t* triFlags;          // may be null (all 0)
  const uint32_t* triAux;            // may be null (all 0)
  uint32_t numVertices;
};
using BvhRefMaker = bool (*)(void* user, const BvhRefInput& in, uint32_t& numRefs, std::string& err);
// Builds the binary tree over n references — binned SAH, stable partitions, median fallback: the decisions, the order of
// the references and the tree of bvh_build.cpp's host code.  nodes[0] is the root; children come after their parents.
//   refs != null (no BvhRefMaker in the backend): refs[0, n) stay as they are; order[i] is the reference (its index = its
//     id) at position i of the leaf order the nodes' ranges speak of, and `nodes` is the whole tree.
//   refs == null: the references the BvhRefMaker of the same `user` kept; order and tree stay there for the BvhPacker,
//     `order` comes back empty and `nodes` holds the root alone.
using BvhTreeBuilder = bool (*)(void* user, const BvhBuildRef* refs, uint32_t n, BigVec<uint32_t>& order, BigVec<BvhBuildNode>& nodes, std::string& err);
// After the collapse: the four-wide nodes as lists of binary nodes, and where each one's index goes in its parent.
struct BvhWideNode {
  uint32_t src;      // binary node this wide node covers
  uint32_t kids[4];  // the binary nodes that became its (up to 4) children
  int32_t nk;
  uint32_t depth;
};
struct BvhSlot {
  int32_t node, idx;  // wide node and child slot that refer to this wide node (-1: the root)
};
struct Bvh;
// Everything after the binary tree — the four-wide collapse, the child boxes quantised, nodes and leaf triangles packed
// into the device's record array — from what the two stages above of the same `user` left behind.  Fills out.deviceRecs /
// out.deviceNumRecs (the caller owns the allocation: hipFree) and out.numNodes / maxDepth / maxStack / sahCost.
struct BvhPackInput {
  uint32_t numTris, numRefs;
  float pad;  // what every child box is padded by before it is quantised
};
using BvhPacker = bool (*)(void* user, const BvhPackInput& in, Bvh& out, std::string& err);
// Where the stages run.  Two shapes besides the empty one (all host code) are legal, and buildBvh refuses any other:
//   buildTree alone             host references, host collapse, host pack (the test hook bdpt_test_tree_builder)
//   makeRefs, buildTree, pack   the whole pipeline (bdpt_set_scene)
struct BvhBackend {
  void* user = nullptr;  // handed to every stage
  BvhRefMaker makeRefs = nullptr;
  BvhTreeBuilder buildTree = nullptr;
  BvhPacker pack = nullptr;
  // The whole pipeline's two forks (measurement knobs of bdpt_set_scene, BDPT_HOST_PRIORITIES / BDPT_UPLOAD_TRI_RECS):
  bool hostPriorities = false;  // the host decides what the clipper leaves, the priorities and the split counts (BvhRefInput::splits / state)
  bool uploadTriRecs = false;   // the host's triangle records and boxes are uploaded (BvhRefInput::uploadTriRecs)
};
// Test hook: the backend buildBvh uses when its options name none (default: the empty one, all host code).
// bdpt_test_tree_builder (api_test.cpp) sets the tree-only shape with the device implementation so that the host-only hash /
// check hooks can be run over a device-built tree and compared with the host-built one.
void bvhSetDefaultBackend(const BvhBackend& b);

// The device implementation (bvh_device.hip).  One BvhDeviceBuild per build: the stages hand their results to one another
// in device memory through it (`user` of the three functions).
struct BvhDeviceBuild;
BvhDeviceBuild* bvhDeviceBuildBegin(int device);
void bvhDeviceBuildEnd(BvhDeviceBuild* b);
// pageable host memory -> the current device through pinned staging buffers and a few copy threads (bvh_device.hip)
bool bvhUploadStaged(void* dst, const void* src, size_t bytes, std::string& err);
// pins the staging buffers of bvhUploadStaged on a thread of its own (once per process; bdpt_create calls it)
void bvhPrewarmStaging(int device);
bool buildBinaryTreeOnDevice(void* user, const BvhBuildRef* refs, uint32_t n, BigVec<uint32_t>& order, BigVec<BvhBuildNode>& nodes, std::string& err);
bool packOnDevice(void* user, const BvhPackInput& in, Bvh& out, std::string& err);
bool makeReferencesOnDevice(void* user, const BvhRefInput& in, uint32_t& numRefs, std::string& err);

struct BvhBuildOptions {
  int threads = 0;                // <= 0: bvhBuildThreads()
  // Spatial pre-splitting (bvh_build.cpp "References"): extra references the builder may create, as a fraction of the
  // number of opaque / non-opaque triangles.  0 = one reference per triangle (object splits only).
  float splitBudget = -1.0f;      // < 0: the build default (BDPT_SPLIT_BUDGET)
  float splitBudgetAlpha = -1.0f; // < 0: the build default (BDPT_SPLIT_BUDGET_ALPHA)
  const BvhRefClipper* clipper = nullptr;  // applied to the pieces of triangles flagged kTriNonOpaque
  uint32_t numVertices = 0;                // vertices `positions` holds (0: unknown; only a backend's reference maker asks)
  const BvhBackend* backend = nullptr;     // null: the default backend (bvhSetDefaultBackend; all host code unless a test set one)
  std::string* error = nullptr;            // receives the message when a backend's stage fails or the backend's shape is illegal (the build is empty then)
};

// positions: 3 floats per vertex; indices: 3 per triangle; triFlags: per triangle (may be null).
// threads <= 0: bvhBuildThreads().  The tree does not depend on the thread count, bit for bit.
void buildBvh(const float* positions, const uint32_t* indices, uint32_t numTriangles, const uint32_t* triFlags, Bvh& out,
              int threads = 0, const uint32_t* triAux = nullptr);
void buildBvh(const float* positions, const uint32_t* indices, uint32_t numTriangles, const uint32_t* triFlags, Bvh& out,
              const BvhBuildOptions& opt, const uint32_t* triAux = nullptr);
// host threads the builder uses by default: BDPT_BUILD_THREADS, else the affinity mask capped by the cgroup CPU quota
int bvhBuildThreads();

// Re-encodes nodes + tris as the 48-byte record array (called by buildBvh; a pure function of the two).
// Returns false when a child block does not fit the format (more than 255 records before a node's last child).
bool packBvh(Bvh& bvh, int threads = 0);

// Decode one quantised plane exactly as the device does.
inline float bvhDecodePlane(const BvhNode& n, int axis, uint8_t q) { return n.origin[axis] + (float)q * n.scale[axis]; }

// ---- one node's quantisation: the host build, the device build (bvh_device.hip k_quantise) and both refits run this ----
// clo / chi: the boxes of the node's nk (0..4) children, already padded.  Writes words 0-9 of the node's record: origin
// (0-2), the biased scale exponents in bits 0-23 of word 3 (bits 24-31, the leaf bits, are cleared: the caller's), the
// 8-bit planes (4-9, BvhNode byte layout; unused slots lo = 255, hi = 0).  Planes round outward.
BVH_HD inline void bvhQuantiseNode(const float (*clo)[3], const float (*chi)[3], int nk, uint32_t* w) {
  float blo[3] = {1e30f, 1e30f, 1e30f}, bhi[3] = {-1e30f, -1e30f, -1e30f};  // node box = union of the padded child boxes
  for (int k = 0; k < nk; k++)
    for (int a = 0; a < 3; a++) {
      blo[a] = clo[k][a] < blo[a] ? clo[k][a] : blo[a];  // std::min(blo, clo)
      bhi[a] = bhi[a] < chi[k][a] ? chi[k][a] : bhi[a];  // std::max(bhi, chi)
    }
  uint32_t ex[3];
  for (int a = 0; a < 3; a++) {
    __builtin_memcpy(&w[a], &blo[a], 4);
    // smallest power of two s with 254 s >= extent (one code of headroom for outward rounding): ext / 254 = m 2^e with
    // m in [0.5, 1) (frexp) — a normal number here (ext >= 1e-30), so e = exponent field - 126
    const float d = bhi[a] - blo[a];
    const float ext = d < 1e-30f ? 1e-30f : d;  // std::max(d, 1e-30f)
    const float q = ext / 254.0f;
    uint32_t qb;
    __builtin_memcpy(&qb, &q, 4);
    int biased = (int)((qb >> 23) & 0xffu) - 126 + 127;
    if (biased < 1) biased = 1;
    if (biased > 254) biased = 254;
    ex[a] = (uint32_t)biased;
    const uint32_t sb = (uint32_t)biased << 23;
    float sc;
    __builtin_memcpy(&sc, &sb, 4);
    uint32_t lo4 = 0, hi4 = 0;
    for (int k = 0; k < 4; k++) {
      if (k >= nk) {
        lo4 |= 255u << (8 * k);
        continue;
      }
      // clamped as floats, then converted: the plain cast of an infinity or a NaN (boxes of positions that overflowed) is
      // undefined on the host and saturates on the device (NaN -> 0); this is the device's answer on both
      const float fl = floorf((clo[k][a] - blo[a]) / sc);
      int ql = !(fl > 0.0f) ? 0 : (fl > 255.0f ? 255 : (int)fl);
      while (ql > 0 && blo[a] + (float)ql * sc > clo[k][a]) ql--;
      const float fh = ceilf((chi[k][a] - blo[a]) / sc);
      int qh = !(fh > 0.0f) ? 0 : (fh > 255.0f ? 255 : (int)fh);
      while (qh < 255 && blo[a] + (float)qh * sc < chi[k][a]) qh++;
      lo4 |= (uint32_t)ql << (8 * k);
      hi4 |= (uint32_t)qh << (8 * k);
    }
    w[4 + a] = lo4;
    w[7 + a] = hi4;
  }
  w[3] = ex[0] | (ex[1] << 8) | (ex[2] << 16);
}

// buildBvh "Triangle records": v0, e1 = v1 - v0, e2 = v2 - v0 of the triangle (a, b, c), and the box of the five points
// (v0, v0 + e1, v0 + e2, v1, v2) with its min / max spelled as BvhBox::grow spells them.
BVH_HD inline void bvhTriGeom(const float* a, const float* b, const float* c, float* v0, float* e1, float* e2, float* lo, float* hi) {
  for (int k = 0; k < 3; k++) {
    const float va = a[k], vb = b[k], vc = c[k];
    v0[k] = va;
    e1[k] = vb - va;
    e2[k] = vc - va;
    const float p1 = v0[k] + e1[k], p2 = v0[k] + e2[k];
    float l = 1e30f, h = -1e30f;
    const float pts[5] = {va, p1, p2, vb, vc};
    for (int j = 0; j < 5; j++) {
      l = pts[j] < l ? pts[j] : l;
      h = h < pts[j] ? pts[j] : h;
    }
    lo[k] = l;
    hi[k] = h;
  }
}
BVH_HD inline float bvhBoxArea(const float* lo, const float* hi) {  // BvhBox::area
  const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
  if (dx < 0 || dy < 0 || dz < 0) return 0.0f;
  return 2.0f * (dx * dy + dy * dz + dz * dx);
}
// Positions the build and the refit are defined for: every |coordinate| <= kBvhMaxCoord = 2^60 (1.15e18).  Up to there no
// box extent, squared diagonal or box area leaves the fp32 range (3 (2^61)^2 < 2^128), so the pad and the SAH cost stay
// finite; bdpt_set_scene and the host-memory updates refuse anything beyond with BDPT_E_INVALID, as they refuse what is
// not finite.  (Device-memory updates are not inspected: beyond the range the pad overflows and every box is NaN — the
// records still hold no address that derives from a position.)
constexpr float kBvhMaxCoord = 1152921504606846976.0f;
BVH_HD inline bool bvhCoordInRange(float x) { return fabsf(x) <= kBvhMaxCoord; }  // (false for a NaN)
// buildBvh's pad from the scene box (the union of the five-point boxes of ALL input triangles): what every child box is
// widened by before it is quantised.  Two terms, the larger one counts:
//   2e-5 of the diagonal   the rounding of the slab test and of the ray / triangle test, both relative to the distances
//                          inside the scene;
//   2^-21 of the largest |coordinate| of the box (at least four ulps of any coordinate)   what is rounded at the size of
//                          the coordinates themselves: the padded plane lo - pad (half an ulp), bvhQuantiseNode's outward
//                          check origin + q scale, which rounds to fp32 while the slab test works on the difference
//                          (origin - ray origin) + q scale without that rounding (half an ulp), and the corners of a
//                          piece box (v0 + u e1) + v e2 (two roundings, one ulp): two ulps, doubled.
// The second term only counts for a scene farther from the origin than 42 of its diagonals; nearer, the pad and every
// record keep the bits of the first term alone.
BVH_HD inline float bvhPadOf(const float* lo, const float* hi, bool any) {
  float diag = 0.0f, big = 0.0f;
  if (any) {
    const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    diag = sqrtf(dx * dx + dy * dy + dz * dz);
    for (int a = 0; a < 3; a++) {
      const float l = fabsf(lo[a]), h = fabsf(hi[a]);
      big = big < l ? l : big;
      big = big < h ? h : big;
    }
  }
  const float rel = 2e-5f * diag + 1e-30f, ulps = 4.76837158203125e-07f * big;
  return rel < ulps ? ulps : rel;
}

// ---- piece-tight refit (BDPT_PREPARE_REFIT_PIECES): a split or clipped reference bounded by its piece ----
// A reference stands for a piece of its triangle, and a per-vertex update maps the triangle affinely: the piece keeps its
// footprint in the triangle's barycentric plane (P = v0 + u e1 + v e2) however the vertices move.  Once, from the tree as
// built, every triangle record gets a region of that plane that contains its piece — the hexagon
//   umin <= u <= umax,  vmin <= v <= vmax,  smin <= u + v <= smax
// around (triangle) n (decoded box of the leaf child the record belongs to): the piece lies in both.  A refit then bounds
// the reference by the hexagon's corners mapped through the moved v0, e1, e2, intersected with the whole triangle's box.
// Six floats per record: umin, umax, vmin, vmax, smin, smax, each widened outward by kPieceMargin and clamped to [0, 1].
// The margin: a hit's (u, v) comes out of the fp32 ray / triangle test with a few ulps of error, and the hexagon's bounds
// lose at most one fp32 rounding (6e-8) when they are stored; 1e-5 is two orders above either, and no more than half the
// pad (2e-5 of the scene diagonal) in world units for the largest triangle a scene can hold.  The boxes also keep the
// refit's `pad`, as every box does.  A reference that is its whole triangle lies inside its leaf's box with `pad` to
// spare, so its region comes out as all of [0, 1] ("whole") and it takes the plain refit's box: a tree without pieces
// gets the plain refit's records.  (That needs `pad` to exceed an ulp of the coordinates, which bvhPadOf's
// second term sees to at any distance from the origin.)
constexpr int kPieceFloats = 6;
constexpr double kPieceMargin = 1e-5;
constexpr int kPiecePolyMax = 12;  // a triangle cut by six half-planes: at most nine vertices
BVH_HD inline bool bvhPieceIsWhole(const float* g) {
  return g[0] <= 0.0f && g[1] >= 1.0f && g[2] <= 0.0f && g[3] >= 1.0f && g[4] <= 0.0f && g[5] >= 1.0f;
}
// The region of the triangle (v0, e1, e2) inside the box [blo, bhi]: the triangle {(0,0), (1,0), (0,1)} clipped in (u, v)
// against the six half-planes lo_a <= v0_a + u e1_a + v e2_a <= hi_a in double precision (Sutherland-Hodgman, as the
// alpha clipper's polygons).  Nothing left (numerically), or anything not finite: the whole triangle.
BVH_HD inline void bvhPieceRegion(const float* v0, const float* e1, const float* e2, const float* blo, const float* bhi, float* g) {
  double pu[kPiecePolyMax], pv[kPiecePolyMax], qu[kPiecePolyMax], qv[kPiecePolyMax];
  int n = 3;
  pu[0] = 0.0, pv[0] = 0.0;
  pu[1] = 1.0, pv[1] = 0.0;
  pu[2] = 0.0, pv[2] = 1.0;
  for (int h = 0; h < 6 && n > 0; h++) {
    const int a = h >> 1;
    // inside: f(u, v) >= 0
    const double sg = (h & 1) ? -1.0 : 1.0;
    const double c0 = sg * ((double)v0[a] - (double)((h & 1) ? bhi[a] : blo[a])), cu = sg * (double)e1[a], cv = sg * (double)e2[a];
    int m = 0;
    for (int i = 0; i < n; i++) {
      const int j = i + 1 == n ? 0 : i + 1;
      const double fi = c0 + pu[i] * cu + pv[i] * cv, fj = c0 + pu[j] * cu + pv[j] * cv;
      const bool ini = fi >= 0.0, inj = fj >= 0.0;
      if (ini && m < kPiecePolyMax) {
        qu[m] = pu[i];
        qv[m] = pv[i];
        m++;
      }
      if (ini != inj && m < kPiecePolyMax) {
        const double t = fi / (fi - fj);
        qu[m] = pu[i] + t * (pu[j] - pu[i]);
        qv[m] = pv[i] + t * (pv[j] - pv[i]);
        m++;
      }
    }
    n = m;
    for (int i = 0; i < n; i++) {
      pu[i] = qu[i];
      pv[i] = qv[i];
    }
  }
  double r[6] = {1e30, -1e30, 1e30, -1e30, 1e30, -1e30};
  for (int i = 0; i < n; i++) {
    const double s = pu[i] + pv[i];
    r[0] = pu[i] < r[0] ? pu[i] : r[0];
    r[1] = r[1] < pu[i] ? pu[i] : r[1];
    r[2] = pv[i] < r[2] ? pv[i] : r[2];
    r[3] = r[3] < pv[i] ? pv[i] : r[3];
    r[4] = s < r[4] ? s : r[4];
    r[5] = r[5] < s ? s : r[5];
  }
  bool ok = n > 0;
  for (int i = 0; i < 6; i++) ok = ok && r[i] >= -1e30 && r[i] <= 1e30;  // (false for a NaN)
  for (int i = 0; i < 6; i++) {
    double x = ok ? r[i] + ((i & 1) ? kPieceMargin : -kPieceMargin) : ((i & 1) ? 1.0 : 0.0);
    x = x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x);
    g[i] = (float)x;
  }
}
// Corner i (0..7) of the hexagon g: (u, max(vmin, smin - u)) and (u, min(vmax, smax - u)) for u = umin, umax, then
// (max(umin, smin - v), v) and (min(umax, smax - v), v) for v = vmin, vmax.  Every vertex of the hexagon lies on a u or a v
// bound, so these eight contain them all.  A range that rounding leaves empty still gives both of its ends: that only
// loosens the box.
BVH_HD inline void bvhPieceCorner(const float* g, int i, float& u, float& v) {
  const float fixed = g[((i >> 2) << 1) + ((i >> 1) & 1)];  // umin, umax, vmin, vmax for i >> 1 = 0..3
  const float olo = g[i & 4 ? 0 : 2], ohi = g[i & 4 ? 1 : 3];  // the other coordinate's own bounds
  float other;
  if (i & 1) {
    const float t = g[5] - fixed;
    other = ohi < t ? ohi : t;
  } else {
    const float t = g[4] - fixed;
    other = olo < t ? t : olo;
  }
  u = i & 4 ? other : fixed;
  v = i & 4 ? fixed : other;
}
// The box of the eight corners mapped through (v0 + u e1) + v e2 in fp32, in corner order, intersected with the box
// (lo, hi) it is handed (the five-point box of the whole triangle), which it overwrites.
BVH_HD inline void bvhPieceBox(const float* v0, const float* e1, const float* e2, const float* g, float* lo, float* hi) {
  const float gg[6] = {g[0], g[1], g[2], g[3], g[4], g[5]};
  float l[3] = {1e30f, 1e30f, 1e30f}, h[3] = {-1e30f, -1e30f, -1e30f};
#ifdef __HIPCC__
#pragma unroll
#endif
  for (int i = 0; i < 8; i++) {
    float u, v;
    bvhPieceCorner(gg, i, u, v);
    for (int a = 0; a < 3; a++) {
      const float p = (v0[a] + u * e1[a]) + v * e2[a];
      l[a] = p < l[a] ? p : l[a];
      h[a] = h[a] < p ? p : h[a];
    }
  }
  for (int a = 0; a < 3; a++) {
    lo[a] = lo[a] < l[a] ? l[a] : lo[a];
    hi[a] = h[a] < hi[a] ? h[a] : hi[a];
  }
}

// ---- refit (bdpt_update_geometry): new vertex positions, the same tree ----
// Everything in the records that derives from positions is rewritten in place; the layout, every record index, leaf bits,
// childBase, child offsets and the prim / flags / aux words of the triangles stay.  A reference is bounded by its whole
// triangle (conservative for split and alpha-clipped pieces), a node by the union of its children, then quantised with
// bvhQuantiseNode and the pad of the new scene box.  The result is a pure function of the built topology and the positions.
// The plan: the four-wide nodes in the order of the build (childBase ascending — packBvh hands the child blocks out in
// node order), grouped by depth so that one pass per level, deepest first, sees every child done.
constexpr uint32_t kRefitLeaf = 0x80000000u;  // BvhRefitNode::kid: leaf child of (kid & ~kRefitLeaf) references
struct BvhRefitNode {
  uint32_t rec;     // record index of the node
  uint32_t nk;      // children
  uint32_t kid[4];  // interior child: its node index (in plan order); leaf child: kRefitLeaf | reference count
};
static_assert(sizeof(BvhRefitNode) == 24, "refit node");
struct BvhRefitPlan {
  std::vector<BvhRefitNode> nodes;  // build order (the SAH sums in this order)
  std::vector<uint32_t> levelOrder;  // node indices, deepest level first
  std::vector<uint32_t> levelStart;  // level l = levelOrder[levelStart[l], levelStart[l + 1])
};
// Derives the plan by a top-down pass over the records (every index checked against numRecs).  false + err when the
// records are not a tree of this format.
bool bvhRefitMakePlan(const BvhRec* recs, size_t numRecs, BvhRefitPlan& plan, std::string& err);
// One node of one level.  box: 6 floats (exact lo, hi) per plan node, read for interior children, written for this one;
// childArea: 4 per plan node (BvhBox::area of each child's exact box, 0 for an unused slot).  The leaf children's
// triangle records are rewritten here too (v0, e1, e2 from prim and the indices).
// PIECES: `region` holds six floats per record (bvhPieceRegion, below "piece-tight refit"); a reference whose region is
// not the whole triangle is bounded by the region's mapped corners instead.  The plain refit is the instance without.
template <bool PIECES>
BVH_HD inline void bvhRefitNodeT(const BvhRefitNode& nd, uint32_t self, BvhRec* recs, const float* pos, const uint32_t* idx, float* box, float* childArea,
                                 float pad, const float* region) {
  float lo[4][3], hi[4][3];
  for (int k = 0; k < 4; k++) {
    if (k >= (int)nd.nk) {
      childArea[(size_t)self * 4 + k] = 0.0f;
      continue;
    }
    const uint32_t kd = nd.kid[k];
    if (kd & kRefitLeaf) {
      BvhRec& parent = recs[nd.rec];
      const uint32_t at = parent.w[10] + ((parent.w[11] >> (8 * k)) & 0xffu);
      for (int a = 0; a < 3; a++) {
        lo[k][a] = 1e30f;
        hi[k][a] = -1e30f;
      }
      for (uint32_t j = 0; j < (kd & ~kRefitLeaf); j++) {
        BvhRec& r = recs[at + j];
        const uint32_t t = r.w[3];
        const float* pa = pos + (size_t)idx[(size_t)t * 3] * 3;
        const float* pb = pos + (size_t)idx[(size_t)t * 3 + 1] * 3;
        const float* pc = pos + (size_t)idx[(size_t)t * 3 + 2] * 3;
        float v0[3], e1[3], e2[3], tl[3], th[3];
        bvhTriGeom(pa, pb, pc, v0, e1, e2, tl, th);
        if constexpr (PIECES) {
          const float* g = region + (size_t)(at + j) * kPieceFloats;
          if (!bvhPieceIsWhole(g)) bvhPieceBox(v0, e1, e2, g, tl, th);
        }
        for (int a = 0; a < 3; a++) {
          __builtin_memcpy(&r.w[a], &v0[a], 4);
          __builtin_memcpy(&r.w[4 + a], &e1[a], 4);
          __builtin_memcpy(&r.w[8 + a], &e2[a], 4);
          lo[k][a] = tl[a] < lo[k][a] ? tl[a] : lo[k][a];  // BvhBox::grow
          hi[k][a] = hi[k][a] < th[a] ? th[a] : hi[k][a];
        }
      }
    } else {
      for (int a = 0; a < 3; a++) {
        lo[k][a] = box[(size_t)kd * 6 + a];
        hi[k][a] = box[(size_t)kd * 6 + 3 + a];
      }
    }
    childArea[(size_t)self * 4 + k] = bvhBoxArea(lo[k], hi[k]);
  }
  float blo[3] = {1e30f, 1e30f, 1e30f}, bhi[3] = {-1e30f, -1e30f, -1e30f};
  float clo[4][3], chi[4][3];
  for (int k = 0; k < (int)nd.nk; k++)
    for (int a = 0; a < 3; a++) {
      blo[a] = lo[k][a] < blo[a] ? lo[k][a] : blo[a];
      bhi[a] = bhi[a] < hi[k][a] ? hi[k][a] : bhi[a];
      clo[k][a] = lo[k][a] - pad;
      chi[k][a] = hi[k][a] + pad;
    }
  for (int a = 0; a < 3; a++) {
    box[(size_t)self * 6 + a] = blo[a];
    box[(size_t)self * 6 + 3 + a] = bhi[a];
  }
  if (nd.nk == 0) return;  // (the one empty node of a scene nothing can hit: nothing to refit)
  uint32_t w[10];
  bvhQuantiseNode(clo, chi, (int)nd.nk, w);
  BvhRec& r = recs[nd.rec];
  for (int i = 0; i < 10; i++) r.w[i] = i == 3 ? (w[3] | (r.w[3] & 0xff000000u)) : w[i];
}
BVH_HD inline void bvhRefitNode(const BvhRefitNode& nd, uint32_t self, BvhRec* recs, const float* pos, const uint32_t* idx, float* box, float* childArea,
                                float pad) {
  bvhRefitNodeT<false>(nd, self, recs, pos, idx, box, childArea, pad, nullptr);
}
BVH_HD inline void bvhRefitNodePieces(const BvhRefitNode& nd, uint32_t self, BvhRec* recs, const float* pos, const uint32_t* idx, float* box,
                                      float* childArea, float pad, const float* region) {
  bvhRefitNodeT<true>(nd, self, recs, pos, idx, box, childArea, pad, region);
}
// The regions of one plan node's leaf children, from the records AS BUILT: the child's box decoded from the node's origin,
// scale exponents and plane bytes (bvhDecodePlane's arithmetic), every one of its references clipped to it.  Writes
// region[kPieceFloats * record] of the triangle records; node records' slots are never read.
BVH_HD inline void bvhPieceRegionsOfNode(const BvhRefitNode& nd, const BvhRec* recs, float* region) {
  const BvhRec& n = recs[nd.rec];
  for (int k = 0; k < (int)nd.nk; k++) {
    const uint32_t kd = nd.kid[k];
    if (!(kd & kRefitLeaf)) continue;
    float blo[3], bhi[3];
    for (int a = 0; a < 3; a++) {
      float org, sc;
      __builtin_memcpy(&org, &n.w[a], 4);
      const uint32_t sb = ((n.w[3] >> (8 * a)) & 0xffu) << 23;
      __builtin_memcpy(&sc, &sb, 4);
      blo[a] = org + (float)((n.w[4 + a] >> (8 * k)) & 0xffu) * sc;
      bhi[a] = org + (float)((n.w[7 + a] >> (8 * k)) & 0xffu) * sc;
    }
    const uint32_t at = n.w[10] + ((n.w[11] >> (8 * k)) & 0xffu);
    for (uint32_t j = 0; j < (kd & ~kRefitLeaf); j++) {
      const BvhRec& r = recs[at + j];
      float v0[3], e1[3], e2[3];
      for (int a = 0; a < 3; a++) {
        __builtin_memcpy(&v0[a], &r.w[a], 4);
        __builtin_memcpy(&e1[a], &r.w[4 + a], 4);
        __builtin_memcpy(&e2[a], &r.w[8 + a], 4);
      }
      bvhPieceRegion(v0, e1, e2, blo, bhi, region + (size_t)(at + j) * kPieceFloats);
    }
  }
}
// Every node's regions on the host (the definition the device's k_refit_regions matches bit for bit).  region: sized by
// it, kPieceFloats per record, zero where no triangle record lies.
void bvhPieceRegionsHost(const BvhRec* recs, size_t numRecs, const BvhRefitPlan& plan, std::vector<float>& region, int threads = 0);
// The SAH cost of a refitted tree with the formula of the build (bvh_build.cpp sahCost, bvh_device.hip k_sah_terms /
// k_sah_sum): float terms, summed in double in node order in blocks of 65536 nodes, the block sums in block order.
float bvhRefitSah(const BvhRefitPlan& plan, const float* rootBox, const float* childArea);
// The whole refit on the host (the definition the device refit matches bit for bit).  box / childArea: sized by it.
// pieces: the regions of bvhPieceRegionsHost for the piece-tight refit, null for the plain one.
void bvhRefitHost(BvhRec* recs, const BvhRefitPlan& plan, const float* positions, const uint32_t* indices, uint32_t numTris,
                  std::vector<float>& box, std::vector<float>& childArea, int threads = 0, const float* pieces = nullptr);

}  // namespace bdpt
