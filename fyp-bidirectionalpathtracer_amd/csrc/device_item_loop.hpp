// device_item_loop.hpp — the persistent item loop of the query kernels (trace_rays.hip, walk_query.hip, ao.hip, gi.hip,
// sky.hip, sky_mis.hip).
//
// Each of those kernels is one wave per workgroup with 64 traversal slots, kStackLds stack rows in LDS and the rest in the
// context's overflow area, and this loop:
//
//   ItemFeed F = feedInit(itemCount(cap, count));
//   while (refill(F, cursor, lane, has, [&](uint32_t item) { /* begin `item`; set `has` unless it is dead */ })) {
//     const bool leavesDue = nodePhase<ORDER>(S, T, stk, active);       // active: the lane holds a ray in flight
//     if (leavesDue && active && T.cur < 0) answered = leafPhase<MODE>(S, T, stk);
//     /* what an answered lane does: store and retire, or start its item's next ray in its own slot
//        (together with the other answered lanes once parkedDue<MIN>() says so) */
//   }
//   releaseCursor(cursor, lane);
//
// What a kernel keeps is what differs: how an item starts and what an answered lane does.  Two kernels keep pieces of
// this loop as their own text, because through the helpers they compiled to other code that measured slower (DESIGN.md
// "The shared item loop"): ao_kernel the fetch, both phases and the gate, gi_kernel the fetch and its two-mode leaf
// step.  Both `continue` where refill returns true for a wave that holds nothing.  A change here is made there too.
// The frame's own kernels (walk_kernel of kernels.hip, trace_shadow_kernel of device_trace.hpp) fetch from sub-queues
// with 32-bit heads and keep their own loops; the leaf schedule below is theirs, and is measured there.
#pragma once
#include "device_trace.hpp"

namespace bdpt {
#define BD __device__ __forceinline__

// Wave-uniform fetch state: the list's length, items per atomic, and the chunk [pos, end) taken from the cursor.
struct ItemFeed {
  uint32_t n, chunk, pos, end;
  bool exhausted;  // the cursor has passed n: nothing left to take
};

// Items go out in chunks of up to kFetchChunk per atomic, but no more than a fair share per wave, rounded up to whole
// waves: a short list still spreads over the grid instead of feeding its first few waves only.
BD ItemFeed feedInit(uint32_t n) {
  const uint32_t share = (n / gridDim.x + kWave - 1) & ~(uint32_t)(kWave - 1);
  ItemFeed F;
  F.n = n;
  F.chunk = share < (uint32_t)kWave ? (uint32_t)kWave : (share > kFetchChunk ? kFetchChunk : share);
  F.pos = F.end = 0;
  F.exhausted = false;
  return F;
}

// Hands items to the lanes without one (`has` false) and says whether the wave goes on: false when the list is exhausted
// and every lane has retired.  Whenever kRefillIdle or more lanes are idle the wave gives them the next items of its
// chunk by ballot + popcount prefix, and takes a new chunk from cursor[0] with ONE atomic when that one is used up, so
// lanes do not idle behind the longest item of a static batch.  cursor[0] is 64 bits wide: every wave adds one chunk
// past the end before it stops, which a 32-bit word could wrap for a list near 2^32.  start(item) is the kernel's "begin
// this item" code, run by the lane that receives it; it sets `has` unless the item is dead (its outputs are written at
// once and the lane stays idle).  A wave that received only dead items holds nothing although the list goes on: the
// call says "go on", the phases below find no lane to work for, and the next call takes the next items.  (A loop in
// here that fetches until a lane holds an item is the same schedule but costs trace_rays_kernel<0, 1> two VGPRs, 81 and
// 82: a wave per SIMD less, and so a smaller persistent grid — DESIGN.md "The shared item loop".)
template <class Start>
BD bool refill(ItemFeed& F, unsigned long long* cursor, int lane, bool& has, Start&& start) {
  const unsigned long long idleMask = __ballot(!has);
  const int idle = __popcll(idleMask);
  if (!F.exhausted && idle >= kRefillIdle) {
    if (F.pos >= F.end) {  // wave-uniform: take a new chunk
      unsigned long long base = 0;
      if (lane == 0) base = atomicAdd(cursor, (unsigned long long)F.chunk);
      base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(base >> 32)) << 32) |
             (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
      if (base < F.n) {
        F.pos = (uint32_t)base;
        F.end = (base + F.chunk < F.n) ? (uint32_t)(base + F.chunk) : F.n;
      } else {
        F.exhausted = true;
      }
    }
    if (!F.exhausted) {
      const uint32_t avail = F.end - F.pos;
      const uint32_t take = ((uint32_t)idle < avail) ? (uint32_t)idle : avail;
      const uint32_t rank = (uint32_t)__popcll(idleMask & ((1ull << lane) - 1ull));
      if (!has && rank < take) start(F.pos + rank);
      F.pos += take;
    }
  }
  return __ballot(has) != 0ull || !F.exhausted;
}

// Node visits of the lanes that hold a ray in flight (`active`), children entered in nodeStep's ORDER; returns whether
// the leaves are due.  Deferred leaves (BDPT_LEAF_WAIT, device_trace.hpp): every active lane takes up to BDPT_NODE_BURST
// visits; a lane that reaches a leaf, or runs out of stack, waits (T.cur < 0), and the leaves are due once
// BDPT_LEAF_WAIT_FRAC8 eighths of the active lanes wait or none can take a visit.  BDPT_LEAF_WAIT 0 is the plain
// while-while form: every lane descends to its leaf, and leaves are always due.  (Why, with timings: the loop of
// trace_shadow_kernel, device_trace.hpp.)
template <int ORDER>
BD bool nodePhase(const SceneDev& S, TravState& T, int* stk, bool active) {
#if BDPT_LEAF_WAIT > 0
  uint32_t nNodes = 0;  // (nodeBurst's tallies: not kept)
  int maxSp = 0;
  nodeBurst<ORDER, kStackLds, BDPT_NODE_BURST, false>(S, T, stk, active, nNodes, maxSp);
  const unsigned long long waitMask = __ballot(active && T.cur < 0), nodeMask = __ballot(active && T.cur >= 0);
  const int waitNeed = (__popcll(waitMask | nodeMask) * BDPT_LEAF_WAIT_FRAC8 + 7) >> 3;
  return (int)__popcll(waitMask) >= waitNeed || nodeMask == 0ull;
#else
  if (active)
    while (T.cur >= 0) nodeStep<ORDER, kStackLds>(S, T, stk);
  return true;
#endif
}

// One leaf of a waiting lane (active, T.cur < 0) as query MODE, then the next stack entry; returns whether the ray is
// answered: its any-hit query ended at this leaf, or its stack is exhausted (T.cur == kDone; T.best holds the answer).
template <int MODE>
BD bool leafPhase(const SceneDev& S, TravState& T, const int* stk) {
  if (T.cur == kDone) return true;
  uint32_t nTris = 0, nAlpha = 0;  // (leafStep's tallies: not kept)
  if (leafStep<MODE, false>(S, T, nTris, nAlpha)) return true;
  T.cur = travPop<kStackLds>(S, T, stk);
  return T.cur == kDone;
}

// Whether the parked lanes — answered, but waiting so that their next step (shading, a new direction) runs for many
// lanes at once — are due: MIN of them wait, or some do and no lane is `traversing`, so nothing else can make progress.
// MIN <= 1: never wait.
template <int MIN>
BD bool parkedDue(bool parked, bool traversing) {
  if (MIN <= 1) return true;
  const unsigned long long parkedMask = __ballot(parked);
  return (int)__popcll(parkedMask) >= MIN || (parkedMask != 0ull && __ballot(traversing) == 0ull);
}

// cursor[0]: next item to hand out, cursor[1]: waves done; both are zero when a launch starts and when it ends.  The
// last wave to finish leaves them at zero for the next launch, so a call (and a graph made of it) is this one kernel
// with no memset ahead of it: a wave counts itself done only after its last chunk — the one that came back past the
// end — so when the count reaches the grid size no wave will touch cursor[0] again.  Waves that never held an item
// count too.
BD void releaseCursor(unsigned long long* cursor, int lane) {
  if (lane == 0) {
    __threadfence();
    if (atomicAdd(&cursor[1], 1ull) == (unsigned long long)gridDim.x - 1ull) {
      cursor[0] = 0ull;
      cursor[1] = 0ull;
    }
  }
}

#undef BD
}  // namespace bdpt
