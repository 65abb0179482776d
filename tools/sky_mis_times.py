"""The MIS sky lighting query (csrc/sky_mis.hip) against the composed loop it replaces and against the plain sky query at
the same ray budget, one item per pixel at 1920x1080 on the bench scene (the 262 k-triangle atrium): the items are the
G-buffer vertices (bdpt_shade_hits' records of the primary hits), the environment is tools/sky_times.py's procedural
2048x1024 sky with a sun.  One JSON line per material (1 Lambertian, 0 GGX) and sample count S (default 1, 8, 32):

  fused_ms   median device time of one Context.sky_lighting_mis call with both techniques (HIP events around it on its stream)
  loop_ms    median device time of the composed loop on the same inputs, wholly on the device and into preallocated
             tensors: per sample env_sample -> bsdf_pdf -> the quotient and clamp -> trace_rays(any) -> a masked add, then
             sample_bsdf -> three LCG steps -> env_eval -> bsdf_pdf -> the quotient and clamp -> trace_rays(any) -> a masked
             add, on one stream; nothing returns to the host
  plain_ms   median device time of Context.sky_lighting (table samples only, Lambertian) with 2 S samples: as many rays
  ratio      loop_ms / fused_ms;  over_plain = fused_ms / plain_ms
  traced     share of the alive items' 2 S terms that are worth a ray; unoccluded: share of those that reach the sky
  equal      fused and loop give the same colour words, counts and final states (checked once, before timing; the loop's
             arithmetic is torch's on the device here, numpy's in tests/test_gpu_sky_mis.py)

The variants run --warmup times, then alternate --reps times in one process; the medians are over those repetitions, with
minimum and maximum beside them.  --fused-only times the fused call alone: for comparing builds of the kernel
(make -C csrc EXTRA=-DBDPT_SKY_MIS_REGEN_MIN=16), one run per build.

--variance instead prints the error at equal sample count: an unoccluded glossy floor (linearRoughness 0.37, specular 0.8,
diffuse 0.2) under the same sky, seen from the sun's mirror direction ("highlight") and from 45 degrees off it ("off"), S
samples with techniques 1 (table), 2 (BSDF) and 3 (both, so twice the rays): mean and variance of the green channel over 64
seeds.

  timeout 900 python tools/sky_mis_times.py [--samples 1,8,32] [--reps 20] [--fused-only] [--variance] [--out FILE]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sky_times import FLT_MAX, H, W, sky_map, timed  # noqa: E402


def lcg3(torch, s):
    """three steps of the pass's LCG on int32 states (two's complement arithmetic wraps as uint32 does)"""
    for _ in range(3):
        s = s * 1664525 + 1013904223
    return s


def variance_lines(torch, pkg, ctx, sp, samples):
    """the floor items: far above the scene, N = +y, so that every direction of the upper hemisphere is unoccluded"""
    f32 = dict(dtype=torch.float32, device="cuda")
    mw, mh = 2048, 1024
    v, u = (mh // 5 + 0.5) / mh, (mw // 3 + 0.5) / mw
    st, ct = math.sin(math.pi * v), math.cos(math.pi * v)
    sun = (-st * math.sin(2 * math.pi * u), ct, st * math.cos(2 * math.pi * u))
    mirror = (-sun[0], sun[1], -sun[2])
    c, s = math.cos(math.pi / 4), math.sin(math.pi / 4)
    off = (mirror[0] * c - mirror[2] * s, mirror[1], mirror[0] * s + mirror[2] * c)  # turned 45 degrees about N
    n = 64
    lines = []
    for view, V in (("highlight", mirror), ("off", off)):
        rec = torch.zeros((n, 24), **f32)
        rec[:, 1] = 1e5
        rec[:, 5], rec[:, 7] = 1.0, 0.37
        rec[:, 8], rec[:, 9], rec[:, 10] = V
        rec[:, 12:15], rec[:, 16:19] = 0.2, 0.8
        seeds = (torch.arange(n, dtype=torch.int32, device="cuda") + 1) * 1103515245
        for S in samples:
            line = {"view": view, "samples": S, "seeds": n}
            for tech in (1, 2, 3):
                col = ctx.sky_lighting_mis(rec, seeds, S, mat_index=0, techniques=tech, stream=sp)
                torch.cuda.synchronize()
                g = col[:, 1].double()
                line[f"mean_{tech}"] = round(float(g.mean()), 5)
                line[f"var_{tech}"] = float(f"{float(g.var(unbiased=True)):.4g}")
            print(json.dumps(line), flush=True)
            lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=262144)
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--samples", default="1,8,32")
    ap.add_argument("--mats", default="1,0")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fused-only", action="store_true", help="time the fused call alone (comparing builds of the kernel)")
    ap.add_argument("--variance", action="store_true", help="the error at equal sample count instead of the timings")
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
    st = torch.cuda.current_stream()
    sp = C.c_void_p(st.cuda_stream)
    f32 = dict(dtype=torch.float32, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    env = sky_map(torch, 2048, 1024)
    ctx.set_environment(env.data_ptr(), 2048, 1024)
    ctx.env_prepare(sp)
    samples = [int(x) for x in args.samples.split(",")]

    if args.variance:
        lines = variance_lines(torch, pkg, ctx, sp, samples)
    else:
        rays0 = ctx.camera_rays(pipe.gbuffer_params(), w, h, stream=sp)
        hits = torch.empty((n, 4), **f32)
        ctx.trace_rays(rays0, "closest_cull_back", out=hits, stream=sp)
        surf = ctx.shade_hits(rays0, hits, True, stream=sp)
        seeds = torch.arange(n, **i32) * 1103515245
        live = surf.view(torch.int32)[:, 23] >= 0
        del rays0, hits
        hi = torch.tensor(FLT_MAX, **f32)
        zero = torch.zeros((), **f32)
        for mat in [int(x) for x in args.mats.split(",")]:
            for S in samples:
                col, counts, sout = torch.empty((n, 4), **f32), torch.empty(n, **i32), torch.empty(n, **i32)
                pcol, pcounts, psout = torch.empty((n, 4), **f32), torch.empty(n, **i32), torch.empty(n, **i32)
                smp, bs, ev, fp = torch.empty((n, 20), **f32), torch.empty((n, 8), **f32), torch.empty((n, 8), **f32), torch.empty((n, 4), **f32)
                vis, rays, dirs = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty((n, 8), **f32), torch.empty((n, 4), **f32)
                rays[:, 3], rays[:, 7] = pipe.min_t, 1e38
                loop = {"sum": torch.empty((n, 3), **f32), "counts": torch.empty(n, **i32), "sout": torch.empty(n, **i32),
                        "col": torch.ones((n, 4), **f32), "traced": torch.zeros((), dtype=torch.int64, device="cuda")}

                def run_fused():
                    ctx.sky_lighting_mis(surf, seeds, S, mat_index=mat, techniques=3, min_t=pipe.min_t, out=col, counts=counts,
                                         seeds_out=sout, stream=sp)

                def run_plain():
                    ctx.sky_lighting(surf, seeds, 2 * S, min_t=pipe.min_t, out=pcol, counts=pcounts, seeds_out=psout, stream=sp)

                def add_term(raw, own_pdf, tally):
                    value = torch.where((own_pdf != 0)[:, None], torch.minimum(torch.where(raw > 0, raw, zero), hi), zero)
                    ctx.trace_rays(rays, "any", out=vis, stream=sp)
                    worth = (value != 0).any(dim=1) & live
                    add = worth & (vis != 0)
                    loop["sum"].add_(torch.where(add[:, None], value, zero))
                    loop["counts"].add_(add)
                    if tally:
                        loop["traced"] += worth.sum()

                def run_loop(tally=False):
                    s = loop["sout"]
                    s.copy_(seeds)
                    loop["counts"].zero_()
                    loop["sum"].zero_()
                    for _ in range(S):
                        ctx.env_sample(surf, s, mat_index=1, min_t=pipe.min_t, out=smp, seeds_out=s, stream=sp)
                        dirs.copy_(smp[:, 4:8])
                        ctx.bsdf_pdf(surf, dirs, mat, out=fp, stream=sp)
                        rays.copy_(smp[:, 0:8])
                        add_term((fp[:, 0:3] * smp[:, 8:11]) / (smp[:, 11] + fp[:, 3])[:, None], smp[:, 11], tally)
                        ctx.sample_bsdf(surf, s, mat, False, out=bs, stream=sp)
                        s.copy_(lcg3(torch, s))
                        dirs.copy_(bs[:, 0:4])
                        ctx.env_eval(dirs, out=ev, stream=sp)
                        ctx.bsdf_pdf(surf, dirs, mat, out=fp, stream=sp)
                        rays[:, 0:3], rays[:, 4:7] = surf[:, 0:3], bs[:, 0:3]
                        add_term((fp[:, 0:3] * ev[:, 0:3]) / (ev[:, 3] + fp[:, 3])[:, None], bs[:, 3], tally)
                    # a dead item takes no draw in the query; the loop advanced its state: put it back
                    s.copy_(torch.where(live, s, seeds))
                    loop["col"][:, 0:3] = torch.where(live[:, None], loop["sum"] / torch.full((), float(S), **f32), surf[:, 12:15])

                run_fused()
                equal, traced = None, 0
                if not args.fused_only:
                    run_loop(tally=True)
                    torch.cuda.synchronize()
                    equal = bool(torch.equal(col.view(torch.int32), loop["col"].view(torch.int32)) and torch.equal(counts, loop["counts"]) and
                                 torch.equal(sout, loop["sout"]))
                    traced = int(loop["traced"])
                variants = (("fused", run_fused), ("loop", run_loop), ("plain", run_plain))[:1 if args.fused_only else 3]
                for _ in range(args.warmup):
                    for _, fn in variants:
                        fn()
                ms = {k: [] for k, _ in variants}
                for _ in range(args.reps):
                    for name, fn in variants:
                        ms[name].append(timed(torch, st, fn))
                med = {k: statistics.median(v) for k, v in ms.items()}
                alive = int(live.sum())
                line = {"n": n, "mat": mat, "samples": S, "fused_ms": round(med["fused"], 3), "fused_min_ms": round(min(ms["fused"]), 3),
                        "fused_max_ms": round(max(ms["fused"]), 3), "alive": round(alive / n, 4)}
                if not args.fused_only:
                    line.update({"loop_ms": round(med["loop"], 3), "loop_min_ms": round(min(ms["loop"]), 3),
                                 "loop_max_ms": round(max(ms["loop"]), 3), "plain_ms": round(med["plain"], 3),
                                 "plain_min_ms": round(min(ms["plain"]), 3), "plain_max_ms": round(max(ms["plain"]), 3),
                                 "ratio": round(med["loop"] / med["fused"], 2), "over_plain": round(med["fused"] / med["plain"], 2),
                                 "equal": equal, "traced": round(traced / max(1, alive * 2 * S), 4),
                                 "unoccluded": round(float(counts[live].sum()) / max(1, traced), 4)})
                print(json.dumps(line), flush=True)
                lines.append(line)
                del col, counts, sout, pcol, pcounts, psout, smp, bs, ev, fp, vis, rays, dirs, loop
    ctx.set_environment()
    pipe.close()
    scene.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
