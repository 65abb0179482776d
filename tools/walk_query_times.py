"""The walk query (csrc/walk_query.hip) against the composed loop it replaces, one eye subpath per pixel at 1920x1080 on the
bench scene (the 262 k-triangle atrium), --steps bounces (default 8).  One JSON line per material model:

  mat        0 GGX, 1 Lambertian
  fused_ms   median device time of one FramePipeline.walk call (HIP events around it on its stream)
  loop_ms    median device time of the composed loop on the same inputs: per bounce trace_rays(closest) -> shade_hits(no
             normal map) -> sample_bsdf into preallocated tensors, and torch glue on the same stream (torch.where and
             multiplies: select the hits, carry payload, colour and direction, write the planes); nothing returns to the host
  ratio      loop_ms / fused_ms
  launches   kernels the loop enqueues per bounce through the library (3); its torch glue comes on top
  *_enqueue_ms
             median host time to enqueue one call of the variant (no synchronise inside): below the device time, the device
             and not the host bounds the variant
  real       share of the steps x items vertices made by a hit
  equal      the two produce the same vertices and info planes, bit for bit (checked once, before timing)

The eye walk starts as the pass's does: eye vertex 1 is bdpt_shade_hits' record of the primary hit, the first direction and
weight are its sample.  Both variants run --warmup times, then alternate --reps times in one process; the medians are over
those repetitions.

  timeout 900 python tools/walk_query_times.py [--steps 8] [--reps 20] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H = 1920, 1080


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=262144)
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    lines = []
    w, h, steps = args.width, args.height, args.steps
    n = w * h
    scene = pkg.Scene.atrium(1, args.triangles)
    for mat in (0, 1):
        pipe = pkg.FramePipeline(scene, w, h, max_depth=1, mat_index=mat)
        ctx = pipe.ctx
        st = torch.cuda.current_stream()
        sp = C.c_void_p(st.cuda_stream)
        f32 = dict(dtype=torch.float32, device="cuda")
        rays = ctx.camera_rays(pipe.gbuffer_params(), w, h, stream=sp)
        hits = torch.empty((n, 4), **f32)
        ctx.trace_rays(rays, "closest_cull_back", out=hits, stream=sp)
        eye = ctx.shade_hits(rays, hits, True, stream=sp)
        seeds = torch.arange(n, dtype=torch.int32, device="cuda") * 1103515245
        s1 = ctx.sample_bsdf(eye, seeds, mat, stream=sp)
        alive = (eye.view(torch.int32)[:, 23] >= 0).to(torch.uint8)
        starts = torch.zeros((n, 12), **f32)
        starts[:, 0:3], starts[:, 3], starts[:, 4:7], starts[:, 7], starts[:, 8:11] = eye[:, 0:3], pipe.min_t, s1[:, 0:3], 1e38, s1[:, 4:7]
        fused = (torch.empty((steps, n, 24), **f32), torch.empty((steps, n, 4), **f32))
        loop_v, loop_i = torch.empty((steps, n, 24), **f32), torch.empty((steps, n, 4), **f32)
        new, smp, ray = torch.empty((n, 24), **f32), torch.empty((n, 8), **f32), torch.empty((n, 8), **f32)
        none = torch.zeros((n, 24), **f32)
        none.view(torch.int32)[:, 23] = -1
        zero3 = torch.zeros((n, 3), **f32)
        STORED, REAL, SPEC = pkg.abi.WALK_STATUS_STORED, pkg.abi.WALK_STATUS_REAL, pkg.abi.WALK_STATUS_SPECULAR

        def run_fused():
            pipe.walk(starts, seeds, steps, alive=alive, out=fused)

        def run_loop():
            payload = torch.zeros((n, 24), **f32)
            payload[:, 0:3] = starts[:, 0:3]
            pspec = torch.zeros(n, dtype=torch.int32, device="cuda")
            pcolor, L, live = starts[:, 8:11], starts[:, 4:7], alive != 0
            for s in range(steps):
                ray[:, 0:3], ray[:, 3], ray[:, 7] = payload[:, 0:3], pipe.min_t, 1e38
                ray[:, 4:7] = torch.where(live[:, None], L, zero3)  # a zero direction: a miss
                ctx.trace_rays(ray, "closest", out=hits, stream=sp)
                ctx.shade_hits(ray, hits, False, out=new, stream=sp)
                ctx.sample_bsdf(new, seeds, mat, out=smp, stream=sp)
                hit = live & (new.view(torch.int32)[:, 23] >= 0)
                payload = torch.where(hit[:, None], new, payload)
                pspec = torch.where(hit, smp.view(torch.int32)[:, 7], pspec)
                pcolor = torch.where(hit[:, None], pcolor * smp[:, 4:7], zero3)
                L = torch.where(hit[:, None], smp[:, 0:3], L)
                loop_v[s] = torch.where(live[:, None], payload, none)
                loop_v[s].view(torch.int32)[:, 23] = torch.where(live, payload.view(torch.int32)[:, 23].clamp(min=0), -1)
                loop_i[s, :, 0:3] = pcolor
                status = torch.where(live, STORED + REAL * hit.to(torch.int32) + SPEC * (pspec != 0).to(torch.int32), 0)
                loop_i[s].view(torch.int32)[:, 3] = status
                live = hit

        run_fused()
        run_loop()
        torch.cuda.synchronize()
        equal = bool(torch.equal(fused[0].view(torch.int32), loop_v.view(torch.int32)) and
                     torch.equal(fused[1].view(torch.int32), loop_i.view(torch.int32)))
        real = float(((fused[1].view(torch.int32)[..., 3] & REAL) != 0).float().mean())
        for _ in range(args.warmup):
            run_fused()
            run_loop()
        ms, host_ms = {"fused": [], "loop": []}, {"fused": [], "loop": []}
        for _ in range(args.reps):
            for name, fn in (("fused", run_fused), ("loop", run_loop)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                t0 = time.perf_counter()
                fn()
                host_ms[name].append((time.perf_counter() - t0) * 1e3)
                e1.record(st)
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        fm, lm = statistics.median(ms["fused"]), statistics.median(ms["loop"])
        line = {"mat": mat, "n": n, "steps": steps, "fused_ms": round(fm, 3), "loop_ms": round(lm, 3), "ratio": round(lm / fm, 2),
                "fused_min_ms": round(min(ms["fused"]), 3), "loop_min_ms": round(min(ms["loop"]), 3), "launches": 3,
                "fused_enqueue_ms": round(statistics.median(host_ms["fused"]), 3),
                "loop_enqueue_ms": round(statistics.median(host_ms["loop"]), 3), "real": round(real, 4), "equal": equal, "mvertices_s": round(real * steps * n / fm / 1e3, 1)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del fused, loop_v, loop_i, new, smp, ray, none, starts, eye, rays, hits
        pipe.close()
    scene.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
