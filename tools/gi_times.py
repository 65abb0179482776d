"""The diffuse GI query (csrc/gi.hip) against the composed loop it replaces, one item per pixel at 1920x1080 on the bench
scene (the 262 k-triangle atrium): the items are the G-buffer vertices (bdpt_shade_hits' records of the primary hits), the
bounce hit is shaded from the camera with the normal map (the pass's setting), the environment is the host's default
colour.  One JSON line per setting (direct only, one bounce with cosine sampling; the fused call also with uniform sampling):

  fused_ms   median device time of one Context.diffuse_gi call (HIP events around it on its stream)
  loop_ms    median device time of the composed loop on the same inputs, wholly on the device and into preallocated
             tensors: sample_lights -> trace_rays(any) -> [sample_bsdf -> trace_rays(closest) -> shade_hits -> sample_lights
             -> trace_rays(any)] with torch glue between them (copies of the rays into contiguous tensors, the two LCG steps
             as one in-place wrapping int32 multiply and add, the masks and the shader's final arithmetic), on one stream;
             nothing returns to the host
  ratio      loop_ms / fused_ms
  *_enqueue_ms
             median host time to enqueue one call of the variant (no synchronise inside)
  equal      fused and loop give the same hits, status words and final states bit for bit, and colours that agree to 1e-5
             relative (torch's fp32 division in the glue is not the kernel's correctly rounded one; tests/test_gpu_gi.py has
             the bit-for-bit comparison, with the arithmetic in numpy), checked once, before timing

The variants run --warmup times, then alternate --reps times in one process; the medians are over those repetitions.
--fused-only times the fused call alone: for comparing builds of the kernel (make -C csrc EXTRA=-DBDPT_GI_SHADE_MIN=32 or
-DBDPT_GI_WAVES_PER_EU=5, its build knobs), one run per build.

  timeout 900 python tools/gi_times.py [--reps 20] [--fused-only] [--out FILE]
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
ENV = (0.5, 0.5, 0.8, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=262144)
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--height", type=int, default=H)
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
    ctx.set_environment(color=ENV)
    st = torch.cuda.current_stream()
    sp = C.c_void_p(st.cuda_stream)
    f32 = dict(dtype=torch.float32, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    rays0 = ctx.camera_rays(pipe.gbuffer_params(), w, h, stream=sp)
    hits0 = torch.empty((n, 4), **f32)
    ctx.trace_rays(rays0, "closest_cull_back", out=hits0, stream=sp)
    surf = ctx.shade_hits(rays0, hits0, True, stream=sp)
    seeds = torch.arange(n, **i32) * 1103515245
    live = surf.view(torch.int32)[:, 23] >= 0
    view = [float(pipe.cam.posW[k]) for k in range(3)]
    del rays0, hits0

    def signed(x):
        x &= 0xFFFFFFFF
        return x - 2**32 if x >= 2**31 else x

    # two nextRand steps in one: s <- a^2 s + (a c + c) mod 2^32, in wrapping int32
    a, c = 1664525, 1013904223
    step_a, step_c = signed(a * a), signed(a * c + c)
    pi = 3.14159265358979323846
    env = torch.tensor(ENV[0:3], **f32)

    # preallocated: the fused call's outputs and the loop's intermediates
    col, hit_o, stat, sout = torch.empty((n, 4), **f32), torch.empty((n, 4), **f32), torch.empty(n, **i32), torch.empty(n, **i32)
    ls1, ls2, s1, s3 = torch.empty((n, 12), **f32), torch.empty((n, 12), **f32), torch.empty(n, **i32), torch.empty(n, **i32)
    ray = torch.empty((n, 8), **f32)
    ray2 = torch.zeros((n, 8), **f32)
    ray2[:, 0:3], ray2[:, 3], ray2[:, 7] = surf[:, 0:3], pipe.min_t, 1e38
    from_view = torch.zeros((n, 8), **f32)
    from_view[:, 0:3] = torch.tensor(view, **f32)
    vis1, vis2 = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    smp, hits, rec2 = torch.empty((n, 8), **f32), torch.empty((n, 4), **f32), torch.empty((n, 24), **f32)
    loop_col, direct, bounce = torch.empty((n, 3), **f32), torch.empty((n, 3), **f32), torch.empty((n, 3), **f32)
    zero3 = torch.zeros((n, 3), **f32)
    nrm, dif = surf[:, 4:7], surf[:, 12:15]

    def term(ls, vis, out):
        occluded = ((ls.view(torch.int32)[:, 11] >> 16) & 1).bool() & (vis == 0)
        torch.where(occluded[:, None], zero3, ls[:, 8:11], out=out)
        return occluded

    def run_fused(indirect, cosine=True):
        ctx.diffuse_gi(surf, seeds, indirect=indirect, cosine=cosine, view_pos=view, normal_map=True, min_t=pipe.min_t, out=col, hits=hit_o,
                       status=stat, seeds_out=sout, stream=sp)

    def run_loop(indirect):
        ctx.sample_lights(surf, seeds, mat_index=1, min_t=pipe.min_t, out=ls1, seeds_out=s1, stream=sp)
        ray.copy_(ls1[:, 0:8])
        ctx.trace_rays(ray, "any", out=vis1, stream=sp)
        occ1 = term(ls1, vis1, direct)
        if not indirect:
            loop_col.copy_(direct)
            return occ1, None, None
        ctx.sample_bsdf(surf, s1, 1, out=smp, stream=sp)
        ray2[:, 4:7] = smp[:, 0:3]
        ctx.trace_rays(ray2, "closest", out=hits, stream=sp)
        ctx.shade_hits(from_view, hits, True, out=rec2, stream=sp)
        torch.mul(s1, step_a, out=s3).add_(step_c)
        ctx.sample_lights(rec2, s3, mat_index=1, min_t=pipe.min_t, out=ls2, stream=sp)
        ray.copy_(ls2[:, 0:8])
        ctx.trace_rays(ray, "any", out=vis2, stream=sp)
        occ2 = term(ls2, vis2, bounce)
        hit = hits.view(torch.int32)[:, 3] >= 0
        torch.where(hit[:, None], bounce, env, out=bounce)
        ndl = (nrm * smp[:, 0:3]).sum(dim=1).clamp_(0.0, 1.0)
        torch.add(direct, ((ndl[:, None] * bounce) * dif / pi) / (ndl / pi)[:, None], out=loop_col)
        return occ1, hit, occ2

    for name, indirect in (("direct", False), ("indirect", True)):
        run_fused(indirect)
        occ1, hit, occ2 = run_loop(indirect)
        torch.cuda.synchronize()
        want_status = occ1.to(torch.int32)
        if indirect:
            want_status = want_status | (hit.to(torch.int32) << 1) | ((hit & occ2).to(torch.int32) << 2)
        both = live & ~torch.isnan(col[:, 0:3]).any(dim=1)
        equal = bool(torch.equal(stat[live], want_status[live]) and torch.equal(sout[live], (s3 if indirect else s1)[live]) and
                     torch.allclose(col[both][:, 0:3], loop_col[both], rtol=1e-5, atol=1e-7))
        if indirect:
            equal = equal and bool(torch.equal(hit_o.view(torch.int32)[live & hit], hits.view(torch.int32)[live & hit]))
        variants = [(name + " fused", lambda: run_fused(indirect))]
        if indirect:
            variants.append((name + " fused uniform", lambda: run_fused(True, cosine=False)))
        if not args.fused_only:
            variants.append((name + " loop", lambda: run_loop(indirect)))
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
        med = {k: statistics.median(v) for k, v in ms.items()}
        f = name + " fused"
        line = {"n": n, "setting": name, "fused_ms": round(med[f], 3), "fused_min_ms": round(min(ms[f]), 3), "fused_max_ms": round(max(ms[f]), 3),
                "fused_enqueue_ms": round(statistics.median(host_ms[f]), 3), "equal": equal, "alive": round(float(live.float().mean()), 4),
                "direct_occluded": round(float(occ1[live].float().mean()), 4)}
        if indirect:
            line.update({"fused_uniform_ms": round(med[name + " fused uniform"], 3), "bounce_hit": round(float(hit[live].float().mean()), 4),
                         "bounce_occluded": round(float((hit & occ2)[live].float().mean()), 4)})
        if not args.fused_only:
            k = name + " loop"
            line.update({"loop_ms": round(med[k], 3), "loop_min_ms": round(min(ms[k]), 3), "loop_max_ms": round(max(ms[k]), 3),
                         "ratio": round(med[k] / med[f], 2), "loop_enqueue_ms": round(statistics.median(host_ms[k]), 3)})
        print(json.dumps(line), flush=True)
        lines.append(line)
    pipe.close()
    scene.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
