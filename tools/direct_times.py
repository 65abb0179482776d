"""The direct lighting query (csrc/direct.hip) against two yardsticks, one item per pixel at 1920x1080 on the bench scene (the
262 k-triangle atrium): the items are the G-buffer vertices (bdpt_shade_hits' records of the primary hits).  The scene's
geometry is lit by tables of 1, 3 and 16 lights (point lights, spot lights with a penumbra and directional lights inside the
scene's bounds, from a fixed seed).  One JSON line per light count:

  fused_ms / fused_hints_ms
             median device time of one Context.direct_lighting call without / with occluder hints (HIP events around it on its
             stream), color, visible and traced all written
  trace_ms   (a) median device time of ONE trace_rays("any") over exactly the rays the kernel traces, gathered beforehand from
             the `traced` masks into one contiguous list: the traversal alone, with no light evaluation and no per-light pass
  loop_ms    (b) median device time of a caller's loop kept wholly on the device, which is what the call replaces.
             bdpt_set_lights keeps a scene's light count, so the loop runs on a second context that holds the same geometry
             with ONE light: per light set_lights([light]) (which re-traces that light's cube map of occluder hints) ->
             sample_lights(mat_index=1) -> a copy of the rays into a contiguous tensor -> trace_rays("any") -> a torch
             accumulate into preallocated tensors; nothing returns to the host
  rays       the rays traced (the set bits of `traced`), and hinted: those the hints settle without a traversal
  equal      the fused colours agree with the loop's sum to 1e-4 relative where the diffuse colour is not near black (the loop
             has no specular fallback, and its pi is M_PI; tests/test_gpu_direct.py has the bit-for-bit comparisons), and
             hints on equals hints off bit for bit on all three outputs; checked once, before timing

The variants run --warmup times, then alternate --reps times in one process; medians, minima and maxima are over those
repetitions.  --fused-only times the fused calls alone: for comparing builds of the kernel (make -C csrc
EXTRA=-DBDPT_DIRECT_KEEP_TERM=0, -DBDPT_DIRECT_ADVANCE_MIN=16 or -DBDPT_DIRECT_WAVES_PER_EU=4, its build knobs), one run per build.

  timeout 900 python tools/direct_times.py [--reps 20] [--lights 1,3,16] [--fused-only] [--out FILE]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H = 1920, 1080


def light_table(abi, count, lo, hi, seed=7):
    """`count` lights inside the box [lo, hi]: point, spot with a penumbra, directional, in turn; intensities scaled with the
    box so that the inverse-square falloff leaves ordinary values"""
    import numpy as np
    rng = np.random.default_rng(seed)
    ext = float(np.max(hi - lo))
    lights = (abi.Light * count)()
    for k in range(count):
        lt = lights[k]
        kind = k % 3
        d = rng.normal(size=3)
        d[1] = -abs(d[1]) - 0.5
        d /= np.linalg.norm(d)
        pos = lo + (hi - lo) * rng.uniform([0.2, 0.5, 0.2], [0.8, 0.9, 0.8])
        for j in range(3):
            lt.posW[j], lt.dirW[j] = float(np.float32(pos[j])), float(np.float32(d[j]))
            lt.intensity[j] = float(np.float32(rng.uniform(0.5, 1.5) * (1.0 if kind == 2 else 0.1 * ext * ext)))
        if kind == 2:
            lt.type = abi.LIGHT_DIRECTIONAL
        else:
            lt.type = abi.LIGHT_POINT
            opening = math.pi if kind == 0 else float(rng.uniform(0.7, 1.2))
            lt.openingAngle = float(np.float32(opening))
            lt.cosOpeningAngle = -1.0 if kind == 0 else float(np.float32(math.cos(float(np.float32(opening)))))
            lt.penumbraAngle = float(np.float32(rng.uniform(0.1, 0.3))) if kind == 1 else 0.0
    return lights


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=262144)
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lights", default="1,3,16", help="the light counts, comma separated (each 1 .. 16)")
    ap.add_argument("--fused-only", action="store_true", help="time the fused calls alone (comparing builds of the kernel)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    abi = pkg.abi
    lines = []
    w, h = args.width, args.height
    n = w * h
    scene = pkg.Scene.atrium(1, args.triangles)
    pipe = pkg.FramePipeline(scene, w, h, max_depth=1, mat_index=1)
    min_t = pipe.min_t
    st = torch.cuda.current_stream()
    sp = C.c_void_p(st.cuda_stream)
    f32 = dict(dtype=torch.float32, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    rays0 = pipe.ctx.camera_rays(pipe.gbuffer_params(), w, h, stream=sp)
    hits0 = torch.empty((n, 4), **f32)
    pipe.ctx.trace_rays(rays0, "closest_cull_back", out=hits0, stream=sp)
    surf = pipe.ctx.shade_hits(rays0, hits0, True, stream=sp)
    torch.cuda.synchronize()
    live = surf.view(torch.int32)[:, 23] >= 0
    del rays0, hits0
    d0 = scene.desc
    verts = np.ctypeslib.as_array(d0.positions, (int(d0.numVertices), 3))
    lo, hi = verts.min(axis=0).astype(np.float64), verts.max(axis=0).astype(np.float64)
    pipe.close()

    col, vis_m, trc_m = torch.empty((n, 4), **f32), torch.empty(n, **i32), torch.empty(n, **i32)
    col_h, vis_h, trc_h = torch.empty((n, 4), **f32), torch.empty(n, **i32), torch.empty(n, **i32)
    ls, ray, acc = torch.empty((n, 12), **f32), torch.empty((n, 8), **f32), torch.empty((n, 3), **f32)
    vis_b = torch.empty(n, dtype=torch.uint8, device="cuda")
    zero3, seeds0 = torch.zeros((n, 3), **f32), torch.zeros(n, **i32)

    for count in [int(x) for x in args.lights.split(",")]:
        lights = light_table(abi, count, lo, hi)
        desc = abi.SceneDesc.from_buffer_copy(d0)
        desc.lights, desc.numLights = lights, count
        one = (abi.Light * 1)(lights[0])
        desc1 = abi.SceneDesc.from_buffer_copy(d0)
        desc1.lights, desc1.numLights = one, 1
        ctx, ctx1 = pkg.Context(0), pkg.Context(0)
        ctx.set_scene(desc)
        ctx1.set_scene(desc1)

        def run_fused(hints):
            if hints:
                ctx.direct_lighting(surf, min_t=min_t, use_hints=True, out=col_h, visible=vis_h, traced=trc_h, stream=sp)
            else:
                ctx.direct_lighting(surf, min_t=min_t, out=col, visible=vis_m, traced=trc_m, stream=sp)

        def run_loop():
            acc.zero_()
            for k in range(count):
                ctx1.set_lights([lights[k]], sp)
                ctx1.sample_lights(surf, seeds0, mat_index=1, min_t=min_t, out=ls, stream=sp)
                ray.copy_(ls[:, 0:8])
                ctx1.trace_rays(ray, "any", out=vis_b, stream=sp)
                occluded = ((ls.view(torch.int32)[:, 11] >> 16) & 1).bool() & (vis_b == 0)
                acc.add_(torch.where(occluded[:, None], zero3, ls[:, 8:11]))

        run_fused(False)
        run_fused(True)
        run_loop()
        torch.cuda.synchronize()
        dif = surf[:, 12:15]
        both = live & ((dif * dif).sum(dim=1) >= 1e-4) & ~torch.isnan(col[:, 0:3]).any(dim=1) & ~torch.isnan(acc).any(dim=1)
        equal = bool(torch.allclose(col[both][:, 0:3], acc[both], rtol=1e-4, atol=1e-6) and torch.equal(col.view(torch.int32), col_h.view(torch.int32))
                     and torch.equal(vis_m, vis_h) and torch.equal(trc_m, trc_h))
        # (a) exactly the rays the kernel traces, and how many of them a hint settles
        parts, hinted = [], 0
        for k in range(count):
            ctx1.set_lights([lights[k]], sp)
            ctx1.sample_lights(surf, seeds0, mat_index=1, min_t=min_t, use_hints=True, out=ls, stream=sp)
            torch.cuda.synchronize()
            pick = ((trc_m >> k) & 1).bool()
            parts.append(ls[pick][:, 0:8].contiguous())
            hinted += int((pick & (((ls.view(torch.int32)[:, 11] >> 16) & 3) == 3)).sum())
        traced_rays = torch.cat(parts) if parts else torch.empty((0, 8), **f32)
        del parts
        vis_a = torch.empty(len(traced_rays), dtype=torch.uint8, device="cuda")

        variants = [("fused", lambda: run_fused(False)), ("fused_hints", lambda: run_fused(True))]
        if not args.fused_only:
            variants += [("trace", lambda: ctx.trace_rays(traced_rays, "any", out=vis_a, stream=sp)), ("loop", run_loop)]
        for _ in range(args.warmup):
            for _, fn in variants:
                fn()
        ms, host_ms = {k: [] for k, _ in variants}, {k: [] for k, _ in variants}
        for _ in range(args.reps):
            for k, fn in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                t0 = time.perf_counter()
                fn()
                host_ms[k].append((time.perf_counter() - t0) * 1e3)
                e1.record(st)
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        line = {"n": n, "lights": count, "alive": round(float(live.float().mean()), 4), "rays": int(len(traced_rays)), "hinted": hinted,
                "equal": equal}
        for k, _ in variants:
            line.update({f"{k}_ms": round(statistics.median(ms[k]), 3), f"{k}_min_ms": round(min(ms[k]), 3), f"{k}_max_ms": round(max(ms[k]), 3),
                         f"{k}_enqueue_ms": round(statistics.median(host_ms[k]), 3)})
        if not args.fused_only:
            line.update({"fused_over_trace": round(line["fused_ms"] / line["trace_ms"], 2), "loop_over_fused": round(line["loop_ms"] / line["fused_ms"], 2)})
        print(json.dumps(line), flush=True)
        lines.append(line)
        torch.cuda.synchronize()
        ctx.close()
        ctx1.close()
    scene.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
