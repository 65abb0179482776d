// texture_planes.h — texel addressing shared by the device samplers (device_scene.hpp) and the host set-up (api_scene.cpp):
// wrap addressing, the power-of-two flags of TexDev, which alpha-test records sample a texture, and the alpha-quad plane.
// Plain C++ apart from the __host__ __device__ markers, so a host-only harness can compile it as it is.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/bdpt.h"

#if defined(__HIPCC__)
#define BDPT_HD __host__ __device__ inline
#else
#define BDPT_HD inline
#endif

namespace bdpt {

// TexDev::pow2: bit 0 set when the width is a power of two, bit 1 when the height is
enum : uint32_t { kTexPow2W = 1u, kTexPow2H = 2u };
BDPT_HD uint32_t texPow2Flags(uint32_t w, uint32_t h) {
  return ((w & (w - 1u)) == 0u ? kTexPow2W : 0u) | ((h & (h - 1u)) == 0u ? kTexPow2H : 0u);
}

// The samplers' float -> int outside the int range (include/bdpt.h "Surface queries"): saturating, NaN -> 0 — what the
// device's convert instruction does with the plain cast of device_scene.hpp.  Host restatements of the samplers
// (alpha_clip.cpp; the CPU oracle has its own copy) convert with this, because the plain cast is undefined there in C++.
BDPT_HD int texelFloorInt(float x0) {
  if (!(x0 == x0)) return 0;
  if (x0 >= 2147483648.0f) return INT32_MAX;
  if (x0 <= -2147483648.0f) return INT32_MIN;
  return (int)x0;
}

// wrap addressing: i mod n in [0, n)
BDPT_HD int wrapi(int i, int n) {
  int m = i % n;
  return (m < 0) ? m + n : m;
}
// The same wrap without a division where the side is a power of two: i & (n - 1) equals wrapi(i, n) for every int i
// (two's complement).  Other sides keep the remainder.
BDPT_HD int wrapT(int i, int n, bool pow2) { return pow2 ? (i & (n - 1)) : wrapi(i, n); }
// wrapi(i + 1, n) for an i already in [0, n)
BDPT_HD int wrapNext(int i, int n) { return (i + 1 == n) ? 0 : i + 1; }

// Whether the alpha test of a non-opaque triangle samples its material's base-colour texture (alpha record mode 2):
// the rule of sampleTexture — every diffuse channel type other than UNUSED and CONST samples, when there is a
// texture.  The record builder (kernels.hip alpha_recs_kernel) and the choice of textures that get an alpha-quad plane
// (api_scene.cpp) both use it, so every mode-2 record has a plane.
BDPT_HD bool alphaSamplesTexture(uint32_t diffuseType, int texBaseColor) {
  return diffuseType != BDPT_CHANNEL_UNUSED && diffuseType != BDPT_CHANNEL_CONST && texBaseColor >= 0;
}

// Rows [y0, y1) of the alpha-quad plane of a w x h RGBA8 texture (device_scene.hpp alphaQuad): per texel (x, y) the alpha
// bytes of its 2x2 bilinear footprint under wrap addressing, a(x, y), a(x+1, y), a(x, y+1), a(x+1, y+1) from the low byte up.
inline void alphaQuadRows(const uint8_t* rgba8, uint32_t w, uint32_t h, uint32_t y0, uint32_t y1, uint32_t* out) {
  for (uint32_t y = y0; y < y1; y++) {
    const uint32_t yn = (uint32_t)wrapNext((int)y, (int)h);
    for (uint32_t x = 0; x < w; x++) {
      const uint32_t xn = (uint32_t)wrapNext((int)x, (int)w);
      const uint32_t a00 = rgba8[((size_t)y * w + x) * 4 + 3], a10 = rgba8[((size_t)y * w + xn) * 4 + 3];
      const uint32_t a01 = rgba8[((size_t)yn * w + x) * 4 + 3], a11 = rgba8[((size_t)yn * w + xn) * 4 + 3];
      out[(size_t)y * w + x] = a00 | (a10 << 8) | (a01 << 16) | (a11 << 24);
    }
  }
}

}  // namespace bdpt
