"""Throughput of the surface queries (csrc/surface_query.hip) per scene and hit set.  One JSON line each:

  scene     the 262 k-triangle atrium (normal and alpha maps), the 262 k-triangle courtyard with alpha-masked foliage
  hits      camera   1920x1080 bdpt_camera_rays traced with back faces culled (the G-buffer pass's primary hits)
            random   4 M incoherent rays (origins uniform in the scene's box, directions uniform) traced closest-hit
  query     shade_nmap (bdpt_shade_hits with BDPT_SHADE_NORMAL_MAP), shade (without), sample / eval (bdpt_bsdf_query,
            GGX, on the records shade_nmap wrote)
  ms        median device time of one call (HIP events around it on its stream) after --warmup calls
  mitems_s  items / ms / 1000
  bytes     algorithmic bytes per item the query streams: shade reads the ray origin and the hit (32 B) and the 112-byte
            shading record and writes the 96-byte surface (material records and texels come on top); sample reads five
            of the record's float4 and the seed (84 B) and writes 32 B; eval reads five float4 and the direction (96 B)
            and writes 16 B.  GB/s = bytes * mitems_s / 1000.

For the camera set one more line puts the split primary pass — camera_rays + trace_rays(closest_cull_back) +
shade_hits(normal map), three kernels — beside bdpt_gbuffer_execute, which does the same work fused into one kernel (and
writes half-precision channels).

  python tools/surface_query_times.py [--scenes atrium,courtyard] [--sets camera,random] [--reps 10] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H = 1920, 1080
BYTES = {"shade_nmap": 32 + 112 + 96, "shade": 32 + 112 + 96, "sample": 80 + 4 + 32, "eval": 80 + 16 + 16}


def random_rays(desc, n, seed=1):
    rng = np.random.default_rng(seed)
    pos = np.ctypeslib.as_array(desc.positions, shape=(desc.numVertices, 3))
    o = rng.uniform(pos.min(axis=0), pos.max(axis=0), (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, np.zeros((n, 1)), d, np.full((n, 1), 1e38)], axis=1).astype(np.float32)


def time_ms(torch, fn, st, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="atrium,courtyard")
    ap.add_argument("--sets", default="camera,random")
    ap.add_argument("--random-rays", type=int, default=4 << 20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    makers = {"atrium": lambda: pkg.Scene.atrium(1, 262144), "courtyard": lambda: pkg.Scene.courtyard(1, 262144)}
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    for name in args.scenes.split(","):
        scene = makers[name]()
        pipe = pkg.FramePipeline(scene, W, H, max_depth=3)
        ctx = pipe.ctx
        st = torch.cuda.current_stream()
        sp = C.c_void_p(st.cuda_stream)
        gp = pipe.gbuffer_params()
        for s in args.sets.split(","):
            if s == "camera":
                rays = ctx.camera_rays(gp, W, H, stream=sp)
                mode = "closest_cull_back"
            else:
                rays = torch.from_numpy(random_rays(scene.desc, args.random_rays)).cuda()
                mode = "closest"
            n = rays.shape[0]
            hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
            ctx.trace_rays(rays, mode, out=hits, stream=sp)
            surf = torch.empty((n, 24), dtype=torch.float32, device="cuda")
            flat = torch.empty((n, 24), dtype=torch.float32, device="cuda")
            ctx.shade_hits(rays, hits, True, out=surf, stream=sp)
            seeds = torch.arange(n, dtype=torch.int32, device="cuda") * 1103515245
            samp = torch.empty((n, 8), dtype=torch.float32, device="cuda")
            ctx.sample_bsdf(surf, seeds, out=samp, stream=sp)
            dirs = torch.cat([samp[:, 0:3], samp[:, 7:8].view(torch.int32).float()], dim=1).contiguous()
            vals = torch.empty((n, 4), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            hit = round(float((hits.view(torch.int32)[:, 3] >= 0).float().mean()), 4)
            calls = {
                "shade_nmap": lambda: ctx.shade_hits(rays, hits, True, out=surf, stream=sp),
                "shade": lambda: ctx.shade_hits(rays, hits, False, out=flat, stream=sp),
                "sample": lambda: ctx.sample_bsdf(surf, seeds, out=samp, stream=sp),
                "eval": lambda: ctx.eval_bsdf(surf, dirs, out=vals, stream=sp),
            }
            for q, fn in calls.items():
                ms = time_ms(torch, fn, st, args.warmup, args.reps)
                mis = n / ms / 1e3
                emit({"scene": name, "hits": s, "n": n, "hit": hit, "query": q, "ms": round(ms, 4), "mitems_s": round(mis, 1),
                      "bytes": BYTES[q], "gb_s": round(BYTES[q] * mis / 1e3, 1)})
            if s == "camera":
                def split():
                    ctx.camera_rays(gp, W, H, out=rays, stream=sp)
                    ctx.trace_rays(rays, mode, out=hits, stream=sp)
                    ctx.shade_hits(rays, hits, True, out=surf, stream=sp)

                ms_split = time_ms(torch, split, st, args.warmup, args.reps)
                ms_cam = time_ms(torch, lambda: ctx.camera_rays(gp, W, H, out=rays, stream=sp), st, args.warmup, args.reps)
                ms_trace = time_ms(torch, lambda: ctx.trace_rays(rays, mode, out=hits, stream=sp), st, args.warmup, args.reps)
                ms_fused = time_ms(torch, lambda: ctx.gbuffer_execute(gp, pipe.gb, sp), st, args.warmup, args.reps)
                emit({"scene": name, "hits": s, "n": n, "query": "split_vs_gbuffer", "split_ms": round(ms_split, 4),
                      "camera_rays_ms": round(ms_cam, 4), "trace_ms": round(ms_trace, 4), "gbuffer_ms": round(ms_fused, 4),
                      "ratio": round(ms_split / ms_fused, 3)})
            del rays, hits, surf, flat, seeds, samp, dirs, vals
        pipe.close()
        scene.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
