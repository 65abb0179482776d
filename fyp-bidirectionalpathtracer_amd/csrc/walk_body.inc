  int* stk = s_stack + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const unsigned long long laneBelow = (1ull << lane) - 1ull;
  const int D = (int)F.p.maxDepth;
  const bool fromLobe = (F.p.flags & BDPT_PARAM_SPECULAR_FROM_LOBE) != 0;
  // the eye walk extends vertices 1..D-1 (none when D < 2), the light walk vertices 0..D-1
  const uint32_t firstV = (D >= 2) ? 0u : kNumSubQueues, numV = 2u * kNumSubQueues - firstV;
  bool trav = false;   // this lane holds a ray
  uint32_t id = 0;     // its path id
  TravState T;
  travInit(T, mk(0), mk(0), F.p.minT, 1.0e38f);
  T.cur = kDone;
  uint32_t nNodes = 0, nTris = 0, nAlpha = 0;
  uint32_t nEye = 0, nLight = 0, nParked = 0, nReady = 0;  // wave-uniform
  uint32_t vq = firstV + blockIdx.x % numV, tried = 0, chunkPos = 0, chunkEnd = 0, chunk = BDPT_WALK_CHUNK;
  bool exhausted = false;
  const uint32_t wavesPerList = (gridDim.x + numV - 1) / numV;
  for (;;) {
    unsigned long long travMask = __ballot(trav);
    // ---- 1. hit / miss shaders, one parked record per lane ------------------------------------------
    // (also when nothing else can make progress: the last records of the wave are shaded short-handed)
    const bool flush = (travMask == 0ull) && nReady == 0 && exhausted && nParked > 0;
    if (nParked >= (uint32_t)BDPT_WALK_SHADE_MIN || flush) {
      const uint32_t n = nParked < (uint32_t)kWave ? nParked : (uint32_t)kWave;
      nParked -= n;
      const bool act = (uint32_t)lane < n;
      uint4 rec = make_uint4(0, 0, 0, 0);
      if (act) rec = s_pool[nParked + (uint32_t)lane];
      __syncthreads();  // the slots may be overwritten by ready rays below
      const uint32_t p = rec.x & 0xffffffu;
      const int path = (int)((rec.x >> 24) & 1u), k = (int)((rec.x >> 25) & 31u);
      nEye += (uint32_t)__popcll(__ballot(act && path == PATH_EYE));
      nLight += (uint32_t)__popcll(__ballot(act && path == PATH_LIGHT));
      bool survive = false;
      f3 L = mk(0);
      if (act) {
        const bool miss = EXT ? (rec.x & kParkedMiss) != 0u : (int)rec.y < 0;
        const int prim = miss ? -1 : (int)rec.y;
        const f3 o = ldPlane3(P, path, k, F_POS, p);
        // what the eye ray that left vertex k found where it ended (EXT): added to the path's pixel below
        f3 found = mk(0);
        bool haveFound = false;
        if (prim >= 0) {
          const uint32_t seed = (path == PATH_EYE) ? P.seedE[p] : P.seedL[p];
          const f3 thr = ldPlane3(P, path, k, F_COL, p);
          Shading sd = shadeHit<false>(S, (uint32_t)prim, __uint_as_float(rec.z), __uint_as_float(rec.w), o);  // V points at WorldRayOrigin()
          float pdf;
          bool isSpec;
          f3 w = sampleBRDF<GGX>(seed, sd.N, sd.N, sd.V, sd.diffuse, sd.specular, sd.roughness, fromLobe, L, pdf, isSpec);
          Vtx v;
          v.color = thr * w;
          v.pos = sd.posW;
          v.N = sd.N;
          v.V = sd.V;
          v.dif = sd.diffuse;
          v.spec = sd.specular;
          v.rough = sd.roughness;
          v.isSpec = isSpec;
          v.pdf = pdf;
          storeVtx(P, path, k + 1, p, v);
          survive = (k + 2 <= D);  // k + 1 < maxK
          if (EXT && path == PATH_EYE && (F.p.flags & BDPT_PARAM_EMISSIVE_HITS) &&
              (sd.emissive.x > 0.0f || sd.emissive.y > 0.0f || sd.emissive.z > 0.0f)) {
            found = thr * sd.emissive;
            haveFound = true;
          }
        } else {
          if (EXT && path == PATH_EYE && (F.p.flags & BDPT_PARAM_ENV_ON_MISS)) {
            const f3 dir = mk(__uint_as_float(rec.y), __uint_as_float(rec.z), __uint_as_float(rec.w));
            const f3 env = F.envMap ? envLookup(F.envMap, F.envW, F.envH, dir) : ld3(F.envColor);
            found = ldPlane3(P, path, k, F_COL, p) * env;
            haveFound = true;
          }
          Vtx g = zeroVtx();
          if (path == PATH_EYE && k == 1) {
            g.pos = o;  // payload still holds initPayload's values (RayPathData.hlsli:69-86)
          } else {
            loadSurf(P, path, k, p, g);
            g.V = ldPlane3(P, path, k, F_V, p);
            if (path == PATH_LIGHT && k == 0) g.pdf = 0.0f;  // initPayload: pdfForward = 0
          }
          g.color = mk(0);
          storeVtx(P, path, k + 1, p, g);
          if (path == PATH_EYE) {
            P.eyeLast[p] = (uint8_t)(k + 1);
          } else {
            P.lightLast[p] = (uint8_t)(k + 1);
            P.lightReal[p] = (uint8_t)k;
          }
        }
        if (MASKED && haveFound && M.mask[P.pix[p]] == 0) haveFound = false;  // a pixel the mask leaves out: `out` stays as it is
        if (EXT && haveFound) {  // path-tracing strategy of k + 1 edges: uniform 1/edges, clamped, no saturate (as NEE terms)
          f3 term = clampVec(found / (float)(k + 1), F.p.clampUpper);
          if (isnan3(term)) term = mk(0);
          float4* out4 = reinterpret_cast<float4*>(F.out);
          const size_t pix = P.pix[p];
          float4 acc = out4[pix];
          acc.x = acc.x + term.x;
          acc.y = acc.y + term.y;
          acc.z = acc.z + term.z;
          acc.w = acc.w + 1.0f;
          out4[pix] = acc;
        }
      }
      // survivors -> ready rays (origin = the stored vertex k+1, re-read at pick-up)
      const unsigned long long sm = __ballot(survive);
      if (survive) {
        const uint32_t slot = kPoolEntries - 1u - nReady - (uint32_t)__popcll(sm & laneBelow);
        s_pool[slot] = make_uint4(packPath(p, path, k + 1), __float_as_uint(L.x), __float_as_uint(L.y), __float_as_uint(L.z));
      }
      nReady += (uint32_t)__popcll(sm);
      // this wave's later loads of the vertices it just stored must see them (same CU: ordering is enough)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __syncthreads();
    }
    // ---- 2. empty lanes take ready rays, then new sub-paths -------------------------------------------
    const int empty = 64 - __popcll(travMask);
    if ((empty >= BDPT_WALK_REFILL || travMask == 0ull) && (nReady > 0 || !exhausted)) {
      const unsigned long long emptyMask = ~travMask;
      const uint32_t rank = (uint32_t)__popcll(emptyMask & laneBelow);
      const uint32_t fromReady = ((uint32_t)empty < nReady) ? (uint32_t)empty : nReady;
      bool got = false;
      uint32_t nid = 0;
      f3 dir = mk(0);
      if (!trav && rank < fromReady) {
        const uint4 r = s_pool[kPoolEntries - nReady + rank];
        nid = r.x;
        dir = mk(__uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w));
        got = true;
      }
      __syncthreads();  // the pool slots just read may be reused by parked records
      nReady -= fromReady;
      uint32_t want = (uint32_t)empty - fromReady;  // lanes still empty: new sub-paths (only reached with nReady == 0)
      uint32_t taken = fromReady;
      while (want > 0 && !exhausted) {
        while (chunkPos >= chunkEnd && !exhausted) {  // wave-uniform loop: take a new chunk
          const uint32_t* counts = (MASKED && vq < kNumSubQueues) ? M.walkEyeCount : P.qcount;
          const uint32_t nq = counts[(vq % kNumSubQueues) * kCursorStride];
          uint32_t base = nq;
          if (__hip_atomic_load(&head[vq * kCursorStride], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < nq) {
            // A sub-path keeps its lane for up to D rays, so the list is handed out in small pieces (BDPT_WALK_CHUNK):
            // with 256 per fetch the last pieces kept single waves busy long after the rest of the grid had drained.
            uint32_t share = (nq / wavesPerList + 15u) & ~15u;
            chunk = share < 16u ? 16u : (share > (uint32_t)BDPT_WALK_CHUNK ? (uint32_t)BDPT_WALK_CHUNK : share);
            if (lane == 0) base = atomicAdd(&head[vq * kCursorStride], chunk);
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
          }
          if (base < nq) {
            chunkPos = base;
            chunkEnd = (base + chunk < nq) ? base + chunk : nq;
            tried = 0;
          } else {
            vq = (vq + 1 == 2u * kNumSubQueues) ? firstV : vq + 1;
            if (++tried >= numV) exhausted = true;
          }
        }
        if (exhausted) break;
        const uint32_t avail = chunkEnd - chunkPos;
        const uint32_t take = (want < avail) ? want : avail;
        if (!trav && !got && rank >= taken && rank < taken + take) {
          const uint32_t* items = (MASKED && vq < kNumSubQueues) ? M.walkEye : P.queue[0];
          const uint32_t p = items[(vq % kNumSubQueues) * P.pathSubCap + chunkPos + (rank - taken)];
          const int path = (int)(vq / kNumSubQueues);
          const float* rd = P.rayDir + (size_t)(path * 3) * P.Np + p;
          nid = packPath(p, path, (path == PATH_EYE) ? 1 : 0);
          dir = mk(rd[0], rd[P.Np], rd[2 * (size_t)P.Np]);
          got = true;
        }
        chunkPos += take;
        taken += take;
        want -= take;
      }
      if (got) {
        id = nid;
        travInit(T, ldPlane3(P, (int)((nid >> 24) & 1u), (int)(nid >> 25), F_POS, nid & 0xffffffu), dir, F.p.minT, 1.0e38f);
        trav = true;
      }
      travMask = __ballot(trav);
    }
    if (travMask == 0ull) {
      if (nParked == 0 && nReady == 0 && exhausted) break;
      continue;  // parked records are flushed (or ready rays picked up) at the top
    }
    // ---- 3. traversal for the lanes that hold a ray
    bool finished = false;
#if BDPT_WALK_LEAF_WAIT > 0
    // node visits in short bursts; a lane that reaches a leaf (or runs out of stack) waits, and the leaves are intersected
    // once half of the lanes that hold a ray are waiting or no lane can take a node visit (device_trace.hpp, trace_shadow_kernel)
    if (trav) {
#pragma unroll 1
      for (int kk = 0; kk < BDPT_WALK_NODE_BURST && T.cur >= 0; kk++) {
        if (COUNT) nNodes++;
        nodeStep<BDPT_WALK_ORDER, kWalkStackLds>(S, T, stk);
      }
    }
    {
      const unsigned long long waitMask = __ballot(trav && T.cur < 0), nodeMask = __ballot(trav && T.cur >= 0);
      const int waitNeed = (__popcll(waitMask | nodeMask) * BDPT_LEAF_WAIT_FRAC8 + 7) >> 3;
      if ((int)__popcll(waitMask) >= waitNeed || nodeMask == 0ull) {
        if (trav && T.cur < 0) {
          finished = (T.cur == kDone);
          if (!finished) {
            finished = leafStep<0, COUNT>(S, T, nTris, nAlpha);
            if (!finished) {
              T.cur = travPop<kWalkStackLds>(S, T, stk);
              finished = (T.cur == kDone);
            }
          }
        }
      }
    }
#else
    if (trav) {
      while (T.cur >= 0) {
        if (COUNT) nNodes++;
        nodeStep<BDPT_WALK_ORDER, kWalkStackLds>(S, T, stk);
      }
      finished = (T.cur == kDone);
      if (!finished) {
        finished = leafStep<0, COUNT>(S, T, nTris, nAlpha);
        if (!finished) {
          T.cur = travPop<kWalkStackLds>(S, T, stk);
          finished = (T.cur == kDone);
        }
      }
    }
#endif
    const unsigned long long finMask = __ballot(finished);
    if (finMask) {
      if (finished) {
        const bool miss = T.best.prim < 0;
        s_pool[nParked + (uint32_t)__popcll(finMask & laneBelow)] =
            (EXT && miss) ? make_uint4(id | kParkedMiss, __float_as_uint(T.d.x), __float_as_uint(T.d.y), __float_as_uint(T.d.z))
                          : make_uint4(id, (uint32_t)T.best.prim, __float_as_uint(T.best.u), __float_as_uint(T.best.v));
        trav = false;
      }
      nParked += (uint32_t)__popcll(finMask);
      __syncthreads();
    }
  }
  if (lane == 0) {
    if (nEye) atomicAdd(&F.counters->v[blockIdx.x % kCounterShards][C_RAYS_EYE], (unsigned long long)nEye);
    if (nLight) atomicAdd(&F.counters->v[blockIdx.x % kCounterShards][C_RAYS_LIGHT], (unsigned long long)nLight);
  }
  if (COUNT) {
    waveAddCount(F.counters, C_NODE_CLOSEST, nNodes);
    waveAddCount(F.counters, C_TRI_CLOSEST, nTris);
    waveAddCount(F.counters, C_ALPHA_CLOSEST, nAlpha);
  }
