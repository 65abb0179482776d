"""The ambient occlusion query (csrc/ao.hip) against the composed loop it replaces, one item per pixel at 1920x1080 on the
bench scene (the 262 k-triangle atrium): the items are the G-buffer vertices (bdpt_shade_hits' records of the primary
hits), the radius is the host pass's default for the scene.  One JSON line per sample count S (default 1, 8, 32):

  fused_ms   median device time of one Context.ambient_occlusion call (HIP events around it on its stream)
  loop_ms    median device time of the composed loop on the same inputs, wholly on the device and into preallocated
             tensors: per sample sample_bsdf(Lambertian) -> one torch copy of the directions into the ray tensor ->
             trace_rays(any) -> one in-place count add, and the two LCG steps as one in-place wrapping int32 multiply and
             one add (five launches per sample), on one stream; nothing returns to the host
  trace_ms   median device time of trace_rays(any) alone, S calls on the same rays generated beforehand: the
             traversal-only floor — what is left of fused_ms is generation and bookkeeping
  ratio      loop_ms / fused_ms;  over_floor = fused_ms / trace_ms
  *_enqueue_ms
             median host time to enqueue one call of the variant (no synchronise inside)
  occluded   share of the rays of alive items that are occluded
  equal      fused and loop give the same ao, counts and final states, bit for bit (checked once, before timing)

The variants run --warmup times, then alternate --reps times in one process; the medians are over those repetitions.
--fused-only times the fused call alone: for comparing builds of the kernel (make -C csrc EXTRA=-DBDPT_AO_GEN_MIN=16,
-DBDPT_AO_RELOAD_N=1 or -DBDPT_AO_WAVES_PER_EU=6, its build knobs), one run per build.

  timeout 900 python tools/ao_times.py [--samples 1,8,32] [--reps 20] [--fused-only] [--out FILE]
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
    ap.add_argument("--samples", default="1,8,32")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fused-only", action="store_true", help="time the fused call alone (comparing builds of the kernel)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    lines = []
    w, h = args.width, args.height
    n = w * h
    scene = pkg.Scene.atrium(1, args.triangles)
    pipe = pkg.FramePipeline(scene, w, h, max_depth=1, mat_index=1)
    ctx = pipe.ctx
    radius = pkg.ao_default_radius(scene.desc)
    st = torch.cuda.current_stream()
    sp = C.c_void_p(st.cuda_stream)
    f32 = dict(dtype=torch.float32, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    rays0 = ctx.camera_rays(pipe.gbuffer_params(), w, h, stream=sp)
    hits = torch.empty((n, 4), **f32)
    ctx.trace_rays(rays0, "closest_cull_back", out=hits, stream=sp)
    surf = ctx.shade_hits(rays0, hits, True, stream=sp)
    seeds = torch.arange(n, **i32) * 1103515245
    live = surf.view(torch.int32)[:, 23] >= 0
    del rays0, hits

    # two nextRand steps in one: s <- a^2 s + (a c + c) mod 2^32, in wrapping int32; a dead item's state stays (1 s + 0)
    def signed(x):
        x &= 0xFFFFFFFF
        return x - 2**32 if x >= 2**31 else x

    a, c = 1664525, 1013904223
    step_a = torch.where(live, signed(a * a), 1).to(torch.int32)
    step_c = torch.where(live, signed(a * c + c), 0).to(torch.int32)

    for S in [int(x) for x in args.samples.split(",")]:
        ao, counts, sout = torch.empty(n, **f32), torch.empty(n, **i32), torch.empty(n, **i32)
        smp, ray, vis = torch.empty((n, 8), **f32), torch.zeros((n, 8), **f32), torch.empty(n, dtype=torch.uint8, device="cuda")
        ray[:, 0:3], ray[:, 3], ray[:, 7] = surf[:, 0:3], pipe.min_t, radius
        all_rays = torch.empty((S, n, 8), **f32)
        loop = {"ao": torch.empty(n, **f32), "counts": torch.empty(n, **i32), "sout": torch.empty(n, **i32)}

        def run_fused():
            ctx.ambient_occlusion(surf, seeds, S, radius, min_t=pipe.min_t, out=ao, counts=counts, seeds_out=sout, stream=sp)

        def run_loop(keep=False):
            s, cnt = loop["sout"], loop["counts"]
            s.copy_(seeds)
            cnt.zero_()
            for k in range(S):
                ctx.sample_bsdf(surf, s, 1, out=smp, stream=sp)  # (a miss record samples a zero direction: its ray misses)
                ray[:, 4:7] = smp[:, 0:3]
                if keep:
                    all_rays[k] = ray
                ctx.trace_rays(ray, "any", out=vis, stream=sp)
                cnt.add_(vis)  # a dead item's rays all miss: its count ends at S, as the query defines it
                s.mul_(step_a).add_(step_c)
            torch.div(cnt, S, out=loop["ao"])

        def run_trace():
            for k in range(S):
                ctx.trace_rays(all_rays[k], "any", out=vis, stream=sp)

        run_fused()
        run_loop(keep=True)
        torch.cuda.synchronize()
        equal = bool(torch.equal(ao.view(torch.int32), loop["ao"].view(torch.int32)) and torch.equal(counts, loop["counts"]) and
                     torch.equal(sout, loop["sout"]))
        occluded = float(1.0 - (counts[live].float().mean() / S))
        variants = (("fused", run_fused), ("loop", run_loop), ("trace", run_trace))[:1 if args.fused_only else 3]
        for _ in range(args.warmup):
            for _, fn in variants:
                fn()
        ms, host_ms = {k: [] for k, _ in variants}, {k: [] for k, _ in variants}
        for _ in range(args.reps):
            for name, fn in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                t0 = time.perf_counter()
                fn()
                host_ms[name].append((time.perf_counter() - t0) * 1e3)
                e1.record(st)
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        med = {k: statistics.median(v) for k, v in ms.items()}
        line = {"n": n, "samples": S, "radius": round(radius, 4), "fused_ms": round(med["fused"], 3),
                "fused_min_ms": round(min(ms["fused"]), 3), "fused_enqueue_ms": round(statistics.median(host_ms["fused"]), 3),
                "occluded": round(occluded, 4), "equal": equal, "alive": round(float(live.float().mean()), 4),
                "mrays_s": round(float(live.sum()) * S / med["fused"] / 1e3, 1)}
        if not args.fused_only:
            line.update({"loop_ms": round(med["loop"], 3), "trace_ms": round(med["trace"], 3), "ratio": round(med["loop"] / med["fused"], 2),
                         "over_floor": round(med["fused"] / med["trace"], 2), "loop_min_ms": round(min(ms["loop"]), 3),
                         "trace_min_ms": round(min(ms["trace"]), 3), "loop_enqueue_ms": round(statistics.median(host_ms["loop"]), 3)})
        print(json.dumps(line), flush=True)
        lines.append(line)
        del ao, counts, sout, smp, ray, vis, all_rays, loop
    pipe.close()
    scene.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
