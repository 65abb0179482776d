// device_item_source.hpp — the item a lane of a fused lighting kernel works on (ao.hip, gi.hip, direct.hip, sky.hip,
// sky_mis.hip): one of a caller's bdpt_surface records (ITEM_SRC_SURFACES, the *_query calls) or one G-buffer pixel of
// the tile (ITEM_SRC_GBUFFER, the *_execute calls).
//
// The contract.  Every helper is a template over the kernel's parameter struct and reads its fields by name; a struct
// that lacks a field a helper names (AoDev has no gbDiffuse) simply never instantiates that helper.  The structs share
// no sub-struct: moving the G-buffer pointers of one changed its kernel's scalar loads and spills (DESIGN.md "The item
// source").  What the fields mean, for all five structs of kernels.h and env_light.h:
//   surf        query: bdpt_surface records, six float4 each: (posW, .) (N, linearRoughness) (V, .) (diffuse, .)
//               (specular, .) (., ., ., prim)
//   alive       query, optional: 0 = the item is dead
//   seeds       query: one RNG state per item                                           [itemSeed]
//   color       query: (colour, 1) per item                                             [itemStoreColor]
//   gbPosition  execute: WorldPosition of the full frame (w != 0: geometry)
//   gbNormal, gbDiffuse, gbSpecRough
//               execute: WorldNormal, MaterialDiffuse, MaterialSpecRough (half4) of the full frame
//   pix         execute: the tile's pixels (PathBuf::pix)
//   frameCount  execute: the seed is initRand(pix, frameCount)                          [itemSeed]
//   out         execute: full-frame RGBA32F, (colour, 1) at the tile's pixels           [itemStoreColor]
//   range       cap, the optional device count and minT; execute: cap = the tile's pixel count, no device word
// A kernel's optional outputs (counts, seedsOut, status, visible, traced) belong to its own store.
#pragma once
#include "device_math.hpp"

namespace bdpt {
#define BD __device__ __forceinline__

enum : int { ITEM_SRC_SURFACES = 0, ITEM_SRC_GBUFFER = 1 };

BD f3 itemHalf3(const uint16_t* base, uint32_t at) {  // xyz of a half4 channel
  const uint2 raw = reinterpret_cast<const uint2*>(base)[at];
  return mk(f16_to_f32((uint16_t)(raw.x & 0xffffu)), f16_to_f32((uint16_t)(raw.x >> 16)), f16_to_f32((uint16_t)(raw.y & 0xffffu)));
}

// Item `i`: whether it is alive, and then its position, and with WITH_N its normal from the same reads (gi_kernel's
// fetch: loaded apart from the position it compiles to another instruction stream).  A record is dead by the caller's
// `alive` byte or a negative prim; a pixel where WorldPosition.w is 0 — the shaders' background branch
// (aoTracing.rt.hlsl:91, simpleDiffuseGI.rt.hlsl:152, lambertianPlusShadows.rt.hlsl:117).
template <int SRC, bool WITH_N, class Dev>
BD bool itemLoad(const Dev& Q, uint32_t i, f3& pos, f3& N) {
  if (SRC == ITEM_SRC_SURFACES) {
    const float4* r = Q.surf + (size_t)i * 6;
    if (Q.alive && Q.alive[i] == 0) return false;
    if (__float_as_int(r[5].w) < 0) return false;
    const float4 q0 = r[0];
    pos = mk(q0.x, q0.y, q0.z);
    if (WITH_N) {
      const float4 q1 = r[1];
      N = mk(q1.x, q1.y, q1.z);
    }
    return true;
  } else {
    const uint32_t fp = Q.pix[i];
    const float4 wp = Q.gbPosition[fp];
    pos = mk(wp.x, wp.y, wp.z);
    if (WITH_N) N = itemHalf3(Q.gbNormal, fp);
    return wp.w != 0.0f;
  }
}
template <int SRC, class Dev>
BD bool itemAlive(const Dev& Q, uint32_t i, f3& pos) {
  f3 unused;
  return itemLoad<SRC, false>(Q, i, pos, unused);
}

template <int SRC, class Dev>
BD f3 itemNormal(const Dev& Q, uint32_t i) {
  if (SRC == ITEM_SRC_SURFACES) {
    const float4 q1 = Q.surf[(size_t)i * 6 + 1];
    return mk(q1.x, q1.y, q1.z);
  }
  return itemHalf3(Q.gbNormal, Q.pix[i]);
}
template <int SRC, class Dev>
BD f3 itemDiffuse(const Dev& Q, uint32_t i) {
  if (SRC == ITEM_SRC_SURFACES) {
    const float4 q3 = Q.surf[(size_t)i * 6 + 3];
    return mk(q3.x, q3.y, q3.z);
  }
  return itemHalf3(Q.gbDiffuse, Q.pix[i]);
}

// The item's RNG state: the caller's, or the pass's initRand(pixel, frameCount, 16) (aoTracing.rt.hlsl:82,
// simpleDiffuseGI.rt.hlsl:149).
template <int SRC, class Dev>
BD uint32_t itemSeed(const Dev& Q, uint32_t i) {
  return (SRC == ITEM_SRC_SURFACES) ? Q.seeds[i] : initRand(Q.pix[i], Q.frameCount);
}

// (colour, 1) to the item's place
template <int SRC, class Dev>
BD void itemStoreColor(const Dev& Q, uint32_t i, f3 color) {
  const float4 c = make_float4(color.x, color.y, color.z, 1.0f);
  if (SRC == ITEM_SRC_SURFACES) {
    Q.color[i] = c;
  } else {
    Q.out[Q.pix[i]] = c;
  }
}

#undef BD
}  // namespace bdpt
