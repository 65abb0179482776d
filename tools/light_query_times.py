"""Throughput of the light queries (csrc/light_query.hip), one item per pixel at 1920x1080.  One JSON line each:

  scene     the Cornell box (a point light and the emissive ceiling patch), the 262 k-triangle atrium (its lamp bodies emit)
  mat       0 GGX, 1 Lambertian
  area      BDPT_PARAM_AREA_LIGHTS: the emitter table is one more light
  query     nee (bdpt_light_query BDPT_LIGHT_NEE), +hints (BDPT_LIGHT_USE_HINTS), +compact (the dense ray list), emit
            (BDPT_LIGHT_EMIT); the surfaces are bdpt_shade_hits' records of the primary hits (eye vertex 1 of the pass)
  ms        median device time of one call (HIP events around it on its stream) after --warmup calls; a compacting call
            includes the memset of its count word
  mitems_s  items / ms / 1000
  bytes     algorithmic bytes per item: NEE reads four (Lambertian) or six (GGX) float4 of the surface and the seed and
            writes the 48-byte sample and the chained seed; a compacted ray adds 36 bytes for the `rays` share of the items
            that append one; EMIT reads the seed and writes 48 + 4.  Light records, the emitter table (a binary search of
            the CDF and one shading record per table sample) and hint triangles come on top.  GB/s = bytes * mitems_s / 1000.
  gen_nee_ms, ratio
            the yardstick: the gen_nee stage of bdpt_execute at maxDepth 1 on the same frame (bdpt_get_stage_times, median of
            --reps frames), which runs the same arithmetic once per pixel and also appends its rays (with hints); ratio =
            ms / gen_nee_ms.

  timeout 600 python tools/light_query_times.py [--scenes cornell,atrium] [--reps 10] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from surface_query_times import time_ms  # noqa: E402

W, H = 1920, 1080


def gen_nee_ms(torch, pipe, warmup, reps):
    pipe.ctx.enable_stage_timing(True)
    ms = []
    for k in range(warmup + reps):
        pipe.render_frame()
        torch.cuda.synchronize()
        t = dict(pipe.ctx.stage_times())
        if k >= warmup:
            ms.append(t["gen_nee"])
    pipe.ctx.enable_stage_timing(False)
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell,atrium")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    a = pkg.abi
    makers = {"cornell": lambda: pkg.Scene.cornell(), "atrium": lambda: pkg.Scene.atrium(1, 262144)}
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    n = W * H
    for name in args.scenes.split(","):
        scene = makers[name]()
        for mat in (0, 1):
            for area in (False, True):
                pipe = pkg.FramePipeline(scene, W, H, max_depth=1, mat_index=mat,
                                         flags=a.PARAM_NO_SPLAT | a.PARAM_NO_CONNECT | (a.PARAM_AREA_LIGHTS if area else 0))
                ctx = pipe.ctx
                st = torch.cuda.current_stream()
                sp = C.c_void_p(st.cuda_stream)
                yard = gen_nee_ms(torch, pipe, args.warmup, args.reps)
                rays = ctx.camera_rays(pipe.gbuffer_params(), W, H, stream=sp)
                hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
                ctx.trace_rays(rays, "closest_cull_back", out=hits, stream=sp)
                surf = ctx.shade_hits(rays, hits, True, stream=sp)
                seeds = torch.arange(n, dtype=torch.int32, device="cuda") * 1103515245
                chain = torch.empty(n, dtype=torch.int32, device="cuda")
                rec = torch.empty((n, 12), dtype=torch.float32, device="cuda")
                cr = torch.empty((n, 8), dtype=torch.float32, device="cuda")
                ci = torch.empty(n, dtype=torch.int32, device="cuda")
                cc = torch.zeros(1, dtype=torch.int32, device="cuda")

                def nee(hints, compact):
                    def run():
                        if compact:
                            cc.zero_()
                        ctx.sample_lights(surf, seeds, mat, pipe.min_t, area, hints, out=rec, seeds_out=chain,
                                          compact=(cr, ci, cc) if compact else None, stream=sp)
                    return run

                calls = {"nee": nee(False, False), "nee+hints": nee(True, False), "nee+compact": nee(False, True),
                         "nee+hints+compact": nee(True, True),
                         "emit": lambda: ctx.emit_lights(seeds, pipe.min_t, area, out=rec, seeds_out=chain, stream=sp)}
                for q, fn in calls.items():
                    ms = time_ms(torch, fn, st, args.warmup, args.reps)
                    torch.cuda.synchronize()
                    status = rec.view(torch.int32)[:, 11] >> 16
                    worth = round(float((status == 1).float().mean()), 4) if q != "emit" else None
                    by = 52 if q == "emit" else (64 if mat else 96) + 4 + 48 + 4 + (36 * worth if "compact" in q else 0)
                    mis = n / ms / 1e3
                    line = {"scene": name, "mat": mat, "area": area, "query": q, "n": n, "ms": round(ms, 4), "mitems_s": round(mis, 1),
                            "bytes": round(by, 1), "gb_s": round(by * mis / 1e3, 1)}
                    if q != "emit":
                        line.update({"rays_worth_tracing": worth, "gen_nee_ms": round(yard, 4), "ratio": round(ms / yard, 3)})
                        if "hints" in q:
                            line["hint_occluded"] = round(float((status >= 2).float().mean()), 4)
                    emit(line)
                del rays, hits, surf, seeds, chain, rec, cr, ci, cc
                pipe.close()
        scene.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
