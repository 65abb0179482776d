// CPU-only sanitizer run (AddressSanitizer + UBSan; GPU sanitizers are not available on the pool): the host-side
// C++ that never touches the device — scene factories, scene loader, BVH builder — and the oracle, driven the way
// the tests drive them.  Built and run by tests/test_sanitizers.py.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../fyp-bidirectionalpathtracer_amd/csrc/bvh.h"
#include "../../fyp-bidirectionalpathtracer_amd/csrc/bvh_refs.h"
#include "../../include/bdpt.h"
#include "../../include/bdpt_scene.h"
#include "../../oracle/bdpt_oracle.h"

static int renderWith(const bdpt_scene_desc& d, const bdpt_camera& cam, uint32_t W, uint32_t H, uint32_t depth, uint32_t mat, uint32_t flags) {
  oracle_scene* s = oracle_scene_create(&d);
  if (!s) return 1;
  const size_t n = (size_t)W * H;
  std::vector<float> pos(n * 4), nrm(n * 4), dif(n * 4), spec(n * 4), extra(n * 4), emis(n * 4), out(n * 4);
  std::vector<uint64_t> splat(n * 4);
  oracle_frame f{};
  f.width = W;
  f.height = H;
  f.y0 = 0;
  f.y1 = H;
  f.worldPosition = pos.data();
  f.worldNormal = nrm.data();
  f.materialDiffuse = dif.data();
  f.materialSpecRough = spec.data();
  f.materialExtra = extra.data();
  f.emissive = emis.data();
  f.out = out.data();
  f.splat = splat.data();
  bdpt_gbuffer_params gp{};
  gp.pixelJitter[0] = gp.pixelJitter[1] = 0.5f;
  gp.focalLen = 1.0f;
  gp.frameCount = 0xdeadbeefu;
  gp.envColor[0] = gp.envColor[1] = 0.5f;
  gp.envColor[2] = 0.8f;
  gp.envColor[3] = 1.0f;
  bdpt_params p{};
  p.minT = 1e-4f;
  p.frameCount = 0x1337;
  p.matIndex = mat;
  p.refractiveIndex = 1.0f;
  p.maxDepth = depth;
  p.emitMult = 1.0f;
  p.clampUpper = 0.9f;
  p.pixelJitter[0] = p.pixelJitter[1] = 0.5f;
  p.flags = flags;
  bdpt_counters cnt{};
  int rc = oracle_gbuffer(s, &cam, &gp, nullptr, &f, 0, 2);
  rc |= oracle_bdpt(s, &cam, &p, &f, 0, 2, &cnt);
  rc |= oracle_resolve(&f);
  // BMFR on top, three frames, regression on
  oracle_bmfr* b = oracle_bmfr_create(W, H);
  for (uint32_t k = 0; k < 3; k++) {
    bdpt_bmfr_params bp{};
    bp.frameNumber = k;
    bp.flags = BDPT_BMFR_PREPROCESS | BDPT_BMFR_REGRESSION | BDPT_BMFR_POSTPROCESS | (k == 2 ? BDPT_BMFR_KEEP_LD_FEATURES | BDPT_BMFR_FULL_FRAME : 0u);
    for (int i = 0; i < 4; i++) bp.prevViewProj[i * 5] = 1.0f;
    rc |= oracle_bmfr_execute(b, &bp, pos.data(), nrm.data(), dif.data(), out.data());
  }
  // mAccumCount has no cap while the camera is still: frame numbers where int arithmetic of the noise-hash index
  // overflows (161,320) and where a signed frame % 16 turns negative (2^31 + 5)
  for (uint32_t frame : {161320u, 2147483653u}) {
    bdpt_bmfr_params bp{};
    bp.frameNumber = frame;
    bp.flags = BDPT_BMFR_PREPROCESS | BDPT_BMFR_REGRESSION | BDPT_BMFR_POSTPROCESS | BDPT_BMFR_KEEP_LD_FEATURES;
    for (int i = 0; i < 4; i++) bp.prevViewProj[i * 5] = 1.0f;
    rc |= oracle_bmfr_execute(b, &bp, pos.data(), nrm.data(), dif.data(), out.data());
  }
  oracle_bmfr_destroy(b);
  oracle_scene_destroy(s);
  double sum = 0;
  for (float v : out) sum += v;
  std::printf("  %ux%u depth %u mat %u: rc=%d rays=%llu sum=%.4f\n", W, H, depth, mat, rc, (unsigned long long)(cnt.raysNee + cnt.raysConnect + cnt.raysSplat), sum);
  return rc;
}

int main(int argc, char** argv) {
  const std::string tmp = argc > 1 ? argv[1] : "/tmp";
  int rc = 0;
  for (int which = 0; which < 3; which++) {
    bdpt_scene* sc = which == 0 ? bdpt_scene_create_cornell() : which == 1 ? bdpt_scene_create_atrium(3, 6000) : bdpt_scene_create_soup(5, 700, 0.2f);
    bdpt_scene_desc d{};
    bdpt_camera cam{};
    rc |= bdpt_scene_get_desc(sc, &d);
    rc |= bdpt_scene_get_camera(sc, 1.5f, &cam);
    bdpt::Bvh bvh;
    bdpt::buildBvh(d.positions, d.indices, d.numTriangles, nullptr, bvh);
    std::printf("scene %d: %u triangles, %zu nodes, stack %u\n", which, d.numTriangles, bvh.nodes.size(), bvh.maxStack);
    if (which < 2) {
      rc |= renderWith(d, cam, 36, 24, 4, 0, 0);
      rc |= renderWith(d, cam, 24, 16, 8, 1, BDPT_PARAM_MIS_POWER);
    }
    bdpt_scene_destroy(sc);
  }
  {  // the full scene build (traversal flags, alpha classification, pre-splitting with clipped pieces) and the host trace hook
    bdpt_scene* sc = bdpt_scene_create_courtyard(2, 9000, 0.6f);
    bdpt_scene_desc d{};
    rc |= bdpt_scene_get_desc(sc, &d);
    for (int variant = 0; variant < 3; variant++) {
      bdpt_bvh_info info{};
      void* h = bdpt_host_bvh_create(&d, 2, variant == 0 ? 0.0f : (variant == 1 ? -1.0f : 2.0f), variant == 0 ? 0.0f : (variant == 1 ? -1.0f : 12.0f),
                                     variant != 0, &info);
      if (!h) {
        rc |= 1;
        continue;
      }
      std::vector<float> rays;
      uint32_t st = 99u;
      auto u01 = [&]() { return (float)((st = st * 1664525u + 1013904223u) >> 8) / 16777216.0f; };
      for (int i = 0; i < 600; i++) {
        const float o[3] = {-13.0f + 26.0f * u01(), 0.2f + 7.0f * u01(), -3.0f + 6.0f * u01()};
        float dd[3] = {u01() - 0.5f, u01() - 0.5f, u01() - 0.5f};
        const float l = std::sqrt(dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2]) + 1e-9f;
        rays.insert(rays.end(), {o[0], o[1], o[2], dd[0] / l, dd[1] / l, dd[2] / l, 1e-4f, 1e38f});
      }
      std::vector<int32_t> prim(600), primScan(600);
      std::vector<float> tuv(1800), tuvScan(1800);
      uint64_t visits[2] = {0, 0};
      for (int mode = 0; mode < 3; mode++) {
        rc |= bdpt_host_bvh_trace(h, rays.data(), 600, mode, 0, 2, prim.data(), tuv.data(), visits);
        rc |= bdpt_host_bvh_trace(h, rays.data(), 600, mode, 1, 2, primScan.data(), tuvScan.data(), nullptr);
        for (int i = 0; i < 600; i++)
          if ((mode == 2 ? (prim[i] >= 0) != (primScan[i] >= 0) : prim[i] != primScan[i]) || tuv[(size_t)i * 3] != tuvScan[(size_t)i * 3]) rc |= 1;
      }
      std::printf("courtyard variant %d: %u references for %u triangles, %u dropped, %u always pass; %llu node visits\n", variant, info.numReferences,
                  info.numTriangles, info.numDropped, info.numAlwaysPass, (unsigned long long)visits[0]);
      bdpt_host_bvh_destroy(h);
    }
    char msg[256] = {0};
    bdpt_bvh_info info{};
    if (bdpt_bvh_build_check(&d, &info, msg, sizeof(msg)) != BDPT_OK) {
      std::printf("build check: %s\n", msg);
      rc |= 1;
    }
    bdpt_scene_destroy(sc);
  }
  {  // buildBvh's backend (bvh.h BvhBackend) on a dozen triangles: a shape that is not legal — a pack stage without a
     // reference maker — is refused with a message before any stage runs; the tree-only shape with a tree builder that
     // fails ends with that stage's message; either way the result is empty
    std::vector<float> pos;
    std::vector<uint32_t> idx;
    for (uint32_t t = 0; t < 12; t++) {
      const float x = (float)t;
      pos.insert(pos.end(), {x, 0.0f, 0.0f, x + 0.5f, 1.0f, 0.0f, x, 0.0f, 1.0f});
      idx.insert(idx.end(), {3 * t, 3 * t + 1, 3 * t + 2});
    }
    static int calls;
    calls = 0;
    const bdpt::BvhTreeBuilder mustNotRun = [](void*, const bdpt::BvhBuildRef*, uint32_t, bdpt::BigVec<uint32_t>&, bdpt::BigVec<bdpt::BvhBuildNode>&, std::string&) -> bool { std::abort(); };
    const bdpt::BvhPacker mustNotPack = [](void*, const bdpt::BvhPackInput&, bdpt::Bvh&, std::string&) -> bool { std::abort(); };
    const bdpt::BvhTreeBuilder failing = [](void*, const bdpt::BvhBuildRef* refs, uint32_t n, bdpt::BigVec<uint32_t>&, bdpt::BigVec<bdpt::BvhBuildNode>&, std::string&) -> bool {
      calls += (refs && n == 12) ? 1 : 100;  // the tree-only shape hands the host's references over
      return false;
    };
    for (int which = 0; which < 2; which++) {
      bdpt::BvhBackend be;
      be.buildTree = which == 0 ? mustNotRun : failing;
      be.pack = which == 0 ? mustNotPack : nullptr;
      std::string error;
      bdpt::BvhBuildOptions opt;
      opt.threads = 2;
      opt.backend = &be;
      opt.error = &error;
      bdpt::Bvh bvh;
      bvh.nodes.resize(3);  // (what an earlier build left must go as well)
      bdpt::buildBvh(pos.data(), idx.data(), 12, nullptr, bvh, opt);
      const bool empty = bvh.nodes.empty() && bvh.tris.empty() && bvh.recs.empty() && !bvh.deviceRecs;
      const bool message = which == 0 ? !error.empty() : error == "tree builder failed";
      std::printf("backend shape %d: \"%s\", %s, %d tree builder calls\n", which, error.c_str(), empty ? "empty" : "NOT EMPTY", calls);
      if (!empty || !message || calls != which) rc |= 1;
    }
  }
  {  // the builders' outward rounding (bvh_refs.h: the next float on the bits, for the host and the device alike) against
     // std::nextafterf: the edges, then a million random doubles of every float magnitude, denormals included
    auto down = [](double x) {
      float f = (float)x;
      if ((double)f > x) f = std::nextafterf(f, -INFINITY);
      return f;
    };
    auto up = [](double x) {
      float f = (float)x;
      if ((double)f < x) f = std::nextafterf(f, INFINITY);
      return f;
    };
    uint64_t tried = 0, wrong = 0;
    auto check = [&](double x) {
      const float d0 = down(x), d1 = bdpt::bvhFloatDown(x), u0 = up(x), u1 = bdpt::bvhFloatUp(x);
      tried++;
      if (std::memcmp(&d0, &d1, 4) != 0 || std::memcmp(&u0, &u1, 4) != 0 || !((double)d1 <= x && x <= (double)u1)) wrong++;
    };
    const float tiny = std::nextafterf(0.0f, 1.0f);  // the smallest denormal
    for (double x : {0.0, 1e-300, 4.9e-324, 1e-60, 0.4 * (double)tiny, 0.5 * (double)tiny, 0.6 * (double)tiny})  // +-0 and what rounds to it
      for (double sgn : {1.0, -1.0}) check(sgn * x);
    for (float f : {tiny, 2.0f * tiny, 12345.0f * tiny, 0.5f * FLT_MIN, std::nextafterf(FLT_MIN, 0.0f), FLT_MIN, 1.0f, std::nextafterf(1.0f, 0.0f), 0.1f,
                    16777216.0f, 3.0e38f, FLT_MAX})
      for (float sgn : {1.0f, -1.0f}) {
        const double x = (double)(sgn * f);
        check(x);  // a float, and one double ulp either side of it
        check(std::nextafter(x, -INFINITY));
        check(std::nextafter(x, INFINITY));
        check(0.5 * (x + (double)std::nextafterf(sgn * f, 0.0f)));  // halfway to its neighbour
      }
    uint64_t st = 0x9e3779b97f4a7c15ull;
    auto rnd = [&]() { return st = st * 6364136223846793005ull + 1442695040888963407ull; };
    for (int i = 0; i < 1000000; i++) {
      const double m = 1.0 + (double)(rnd() >> 11) / 9007199254740992.0;  // [1, 2), all 52 mantissa bits
      const int e = (int)((rnd() >> 33) % 279u) - 151;                    // 2^-151 (below the denormals) .. 2^127
      const double x = std::ldexp((rnd() >> 63) ? -m : m, e);
      if (std::fabs(x) <= (double)FLT_MAX) check(x);
    }
    std::printf("outward rounding: %llu values, %llu differ from nextafterf\n", (unsigned long long)tried, (unsigned long long)wrong);
    if (wrong || tried < 900000) rc |= 1;
  }
  {  // scene loader on a small OBJ + MTL + PPM
    std::ofstream(tmp + "/san.mtl") << "newmtl a\nKd 0.5 0.6 0.7\nKs 0.1 0.1 0.1\nNs 0.4\nmap_Kd san.ppm\nnewmtl b.DoubleSided\nKe 1 1 1\n";
    {
      std::ofstream ppm(tmp + "/san.ppm", std::ios::binary);
      ppm << "P6\n2 2\n255\n";
      const unsigned char px[12] = {255, 0, 0, 0, 255, 0, 0, 0, 255, 255, 255, 255};
      ppm.write(reinterpret_cast<const char*>(px), 12);
    }
    std::ofstream(tmp + "/san.obj") << "mtllib san.mtl\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0 0 1\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nusemtl a\nf 1/1 2/2 3/3 4/4\n"
                                      "usemtl b.DoubleSided\nf -1 -4 -3\nusemtl nope\nf 1 5 2\n";
    std::ofstream(tmp + "/san.fscene") << "{ \"models\": [ { \"file\": \"san.obj\", \"instances\": [ { \"translation\": [1,2,3], \"rotation\": [10,20,30], \"scaling\": [1,2,1] } ] } ],"
                                         " \"lights\": [ { \"type\": \"point_light\", \"pos\": [0,3,0], \"direction\": [0,-1,0], \"intensity\": [5,5,5], \"opening_angle\": 45.0, \"penumbra_angle\": 3.0 } ],"
                                         " \"cameras\": [ { \"name\": \"c\", \"pos\": [0,1,5], \"target\": [0,0,0], \"up\": [0,1,0], \"focal_length\": 30.0 } ] }";
    char msg[256] = {0};
    bdpt_scene* sc = bdpt_scene_load((tmp + "/san.fscene").c_str(), msg, sizeof(msg));
    if (!sc) {
      std::printf("loader failed: %s\n", msg);
      rc |= 1;
    } else {
      bdpt_scene_desc d{};
      bdpt_camera cam{};
      bdpt_scene_get_desc(sc, &d);
      bdpt_scene_get_camera(sc, 1.0f, &cam);
      std::printf("loaded: %u triangles %u materials %u textures %u lights\n", d.numTriangles, d.numMaterials, d.numTextures, d.numLights);
      rc |= renderWith(d, cam, 16, 16, 3, 0, 0);
      bdpt_scene_destroy(sc);
    }
    bdpt_scene* bad = bdpt_scene_load((tmp + "/missing.fscene").c_str(), msg, sizeof(msg));
    if (bad) rc |= 1;
  }
  {  // the threaded OBJ reader on mutated and truncated model text (host/SceneLoader.cpp parses raw memory with memchr /
     // from_chars): a corrupt file may be refused or load as something else, never read or write out of bounds; and an
     // intact one gives the same scene for 1, 3 and 8 threads
    std::string good = "mtllib san.mtl\n# comment\nv 0 0 0\nv 1 0 0\r\nv 1 1 0\nv 0 1 0\nv 0 0 1\nvn 0 0 1\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nusemtl a\n"
                       "f 1/1/1 2/2/1 3/3/1 4/4/1\nusemtl b.DoubleSided\nf -1 -4 -3\nf 1//1 5//1 2//1\ng grp\ns off\nusemtl nope\nf 1 5 2 3 4\nf +1 2 3\n";
    for (int k = 0; k < 400; k++) good += "v " + std::to_string(k % 7) + ".5 " + std::to_string(k % 5) + " -" + std::to_string(k % 3) + "e-1\nf -1 -2 -3\n";
    uint32_t state = 777u;
    auto rnd = [&]() { return state = state * 1664525u + 1013904223u; };
    int loaded = 0, refused = 0;
    uint32_t trisGood[3] = {0, 0, 0};
    for (int k = 0; k < 600; k++) {
      std::string d = good;
      if (k >= 3) {
        const int flips = 1 + (int)(rnd() % 6);
        static const char pool[] = "0123456789-+/. \n\rvftnemusl#e";
        for (int i = 0; i < flips; i++) d[rnd() % d.size()] = (rnd() % 3) ? pool[rnd() % (sizeof(pool) - 1)] : (char)(rnd() >> 24);
        if (k % 4 == 0) d.resize(1 + rnd() % d.size());
      }
      std::ofstream(tmp + "/mut.obj", std::ios::binary).write(d.data(), (std::streamsize)d.size());
      bdpt_scene_load_threads(k % 3 == 0 ? 1 : (k % 3 == 1 ? 3 : 8));
      char msg[256] = {0};
      bdpt_scene* sc = bdpt_scene_load((tmp + "/mut.obj").c_str(), msg, sizeof(msg));
      if (sc) {
        bdpt_scene_desc dd{};
        bdpt_scene_get_desc(sc, &dd);
        for (uint32_t t = 0; t < dd.numTriangles * 3; t++)
          if (dd.indices[t] >= dd.numVertices) rc |= 1;  // whatever was loaded is a consistent scene
        if (k < 3) trisGood[k] = dd.numTriangles;
        loaded++;
        bdpt_scene_destroy(sc);
      } else {
        refused++;
        if (k < 3) rc |= 1;  // the unmodified file must load
      }
    }
    bdpt_scene_load_threads(0);
    if (trisGood[0] == 0 || trisGood[0] != trisGood[1] || trisGood[0] != trisGood[2]) rc |= 1;
    std::printf("obj reader: %d loaded, %d refused, %u triangles in the intact file\n", loaded, refused, trisGood[0]);
  }
  {  // image decoders: the files tests/test_sanitizers.py wrote, then byte-mutated and truncated copies of them (a corrupt
     // file may be refused or decoded to garbage, never read or written out of bounds)
    uint32_t state = 12345u;
    auto rnd = [&]() { return state = state * 1664525u + 1013904223u; };
    int decoded = 0, refused = 0;
    for (const char* name : {"san_rgba.png", "san_pal.png", "san_420.jpg", "san_grey.jpg", "san_rst.jpg", "san_probe.hdr"}) {
      const bool hdr = std::strstr(name, ".hdr") != nullptr;
      std::ifstream f(tmp + "/" + name, std::ios::binary);
      if (!f) continue;
      std::vector<char> good((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
      for (int k = 0; k < 400; k++) {
        std::vector<char> d = good;
        if (k > 0) {
          const int flips = 1 + (int)(rnd() % 4);
          for (int i = 0; i < flips; i++) d[rnd() % d.size()] = (char)(rnd() >> 24);
          if (k % 5 == 0) d.resize(1 + rnd() % d.size());
        }
        const std::string path = tmp + "/mut.bin";
        std::ofstream(path, std::ios::binary).write(d.data(), (std::streamsize)d.size());
        uint32_t w = 0, h = 0, a = 0;
        char msg[128];
        if (hdr) {  // the light-probe reader (Radiance RGBE)
          if (bdpt_image_load_hdr(path.c_str(), &w, &h, nullptr, 0, msg, sizeof(msg)) == BDPT_OK) {
            std::vector<float> px((size_t)w * h * 4);
            if (bdpt_image_load_hdr(path.c_str(), &w, &h, px.data(), px.size(), msg, sizeof(msg)) != BDPT_OK) rc |= 1;
            decoded++;
          } else {
            refused++;
            if (k == 0) rc |= 1;
          }
          continue;
        }
        if (bdpt_image_load(path.c_str(), &w, &h, &a, nullptr, 0, msg, sizeof(msg)) == BDPT_OK) {
          std::vector<uint8_t> px((size_t)w * h * 4);
          if (bdpt_image_load(path.c_str(), &w, &h, &a, px.data(), px.size(), msg, sizeof(msg)) != BDPT_OK) rc |= 1;
          decoded++;
        } else {
          refused++;
          if (k == 0) rc |= 1;  // the unmodified file must decode
        }
      }
    }
    std::printf("image decoders: %d decoded, %d refused\n", decoded, refused);
  }
  std::printf("sanitizer run finished rc=%d\n", rc);
  return rc;
}
