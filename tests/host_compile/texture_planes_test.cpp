// Host harness for csrc/texture_planes.h (tests/test_texel_fetch_exact.py): runs the header's own code on inputs the
// test writes and writes what it computes, for the test to compare against the old addressing formula.
//   texture_planes_test plane IN OUT      IN: uint32 w, h, then w*h RGBA8 texels    OUT: w*h uint32 (alphaQuadRows)
//   texture_planes_test wrap N IN OUT     IN: int32 coordinates    OUT: per coordinate int32 wrapT(i, N, pow2), wrapNext(that, N),
//                                         pow2 from texPow2Flags(N, N)
//   texture_planes_test flags             prints "w h flags" for a list of sides
//   texture_planes_test floor IN OUT      IN: float32 values x0 = floorf(x)    OUT: per value int32 texelFloorInt(x0)
//   texture_planes_test rule              prints "type tex alphaSamplesTexture" for every 3-bit diffuse type
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "texture_planes.h"

using namespace bdpt;

static std::vector<unsigned char> readAll(const char* path) {
  std::vector<unsigned char> v;
  FILE* f = std::fopen(path, "rb");
  if (!f) std::exit(2);
  unsigned char buf[65536];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
  std::fclose(f);
  return v;
}
static void writeAll(const char* path, const void* p, size_t n) {
  FILE* f = std::fopen(path, "wb");
  if (!f || std::fwrite(p, 1, n, f) != n) std::exit(3);
  std::fclose(f);
}

int main(int argc, char** argv) {
  if (argc >= 4 && !std::strcmp(argv[1], "plane")) {
    const std::vector<unsigned char> in = readAll(argv[2]);
    uint32_t wh[2];
    std::memcpy(wh, in.data(), 8);
    if (in.size() != 8 + (size_t)wh[0] * wh[1] * 4) return 4;
    std::vector<uint32_t> out((size_t)wh[0] * wh[1]);
    // in two row ranges, as the host threads split it
    const uint32_t mid = wh[1] / 2;
    alphaQuadRows(in.data() + 8, wh[0], wh[1], 0, mid, out.data());
    alphaQuadRows(in.data() + 8, wh[0], wh[1], mid, wh[1], out.data());
    writeAll(argv[3], out.data(), out.size() * 4);
    return 0;
  }
  if (argc >= 5 && !std::strcmp(argv[1], "wrap")) {
    const int n = std::atoi(argv[2]);
    const std::vector<unsigned char> in = readAll(argv[3]);
    const size_t m = in.size() / 4;
    std::vector<int32_t> x(m), out(2 * m);
    std::memcpy(x.data(), in.data(), m * 4);
    const bool pow2 = (texPow2Flags((uint32_t)n, (uint32_t)n) & kTexPow2W) != 0u;
    for (size_t i = 0; i < m; i++) {
      out[2 * i] = wrapT(x[i], n, pow2);
      out[2 * i + 1] = wrapNext(out[2 * i], n);
    }
    writeAll(argv[4], out.data(), out.size() * 4);
    return 0;
  }
  if (argc >= 4 && !std::strcmp(argv[1], "floor")) {
    const std::vector<unsigned char> in = readAll(argv[2]);
    const size_t m = in.size() / 4;
    std::vector<float> x(m);
    std::vector<int32_t> out(m);
    std::memcpy(x.data(), in.data(), m * 4);
    for (size_t i = 0; i < m; i++) out[i] = texelFloorInt(x[i]);
    writeAll(argv[3], out.data(), out.size() * 4);
    return 0;
  }
  if (argc >= 2 && !std::strcmp(argv[1], "flags")) {
    const uint32_t sides[][2] = {{1, 1}, {1, 7}, {7, 1}, {2, 3}, {3, 2}, {256, 256}, {512, 100}, {100, 512}, {1000, 1024}, {96, 128}};
    for (const auto& s : sides) std::printf("%u %u %u\n", s[0], s[1], texPow2Flags(s[0], s[1]));
    return 0;
  }
  if (argc >= 2 && !std::strcmp(argv[1], "rule")) {
    for (uint32_t type = 0; type < 8; type++)
      for (int tex = -1; tex <= 0; tex++) std::printf("%u %d %d\n", type, tex, alphaSamplesTexture(type, tex) ? 1 : 0);
    return 0;
  }
  return 1;
}
