"""Throughput of the connection queries (csrc/connect_query.hip), one item per pixel at 1920x1080 on the bench scene (the
262 k-triangle atrium).  One JSON line each:

  mat       0 GGX, 1 Lambertian
  query     vertices (bdpt_connect_query BDPT_CONNECT_VERTICES with both predecessors), camera (BDPT_CONNECT_CAMERA), each
            also +compact (the dense ray list); splat_add (bdpt_splat_add over every item, every entry landing: items
            without a pixel target their own index), splat_add hot pixel (those items all target pixel 0 instead: the
            contended case), splat_add+items (over CAMERA mode's compact list with its device count and the visibility
            bytes of the any-hit trace)
            The eye vertices are bdpt_shade_hits' records of the primary hits (eye vertex 1 of the pass), the light vertices
            light vertex 1 of one light subpath per pixel: emit_lights -> trace_rays(closest) -> shade_hits.
  ms        median device time of one call (HIP events around it on its stream) after --warmup calls; a compacting call
            includes the memset of its count word
  mitems_s  items / ms / 1000 (splat_add+items: list entries)
  bytes     algorithmic bytes per item.  VERTICES reads two records (three float4 each plus the prim's float4 for
            Lambertian, five plus the prim's for GGX), two 16-byte predecessors (GGX) and writes 48; CAMERA reads one record
            and writes 64; a compacted ray adds 36 bytes for the share of the items that append one.  splat_add reads 4 + 16
            (+ 1 visible, + 4 items) and does up to four 8-byte atomics per landed entry.  GB/s = bytes * mitems_s / 1000.
  trace_any_ms
            the trace call the compact list feeds (bdpt_trace_rays BDPT_TRACE_ANY over it with its device count), for scale

  timeout 600 python tools/connect_query_times.py [--reps 10] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from surface_query_times import time_ms  # noqa: E402

W, H = 1920, 1080


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=262144)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    n = W * H
    scene = pkg.Scene.atrium(1, args.triangles)
    for mat in (0, 1):
        pipe = pkg.FramePipeline(scene, W, H, max_depth=1, mat_index=mat)
        ctx = pipe.ctx
        st = torch.cuda.current_stream()
        sp = C.c_void_p(st.cuda_stream)
        rays = ctx.camera_rays(pipe.gbuffer_params(), W, H, stream=sp)
        hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        ctx.trace_rays(rays, "closest_cull_back", out=hits, stream=sp)
        eye = ctx.shade_hits(rays, hits, True, stream=sp)
        eye_prev = rays[:, 0:4].contiguous()
        seeds = torch.arange(n, dtype=torch.int32, device="cuda") * 1103515245
        em = ctx.emit_lights(seeds, pipe.min_t, stream=sp)
        lrays = em[:, 0:8].contiguous()
        ctx.trace_rays(lrays, "closest", out=hits, stream=sp)
        light = ctx.shade_hits(lrays, hits, False, stream=sp)
        light_prev = lrays[:, 0:4].contiguous()
        rec = torch.empty((n, 12), dtype=torch.float32, device="cuda")
        cam = torch.empty((n, 16), dtype=torch.float32, device="cuda")
        cr = torch.empty((n, 8), dtype=torch.float32, device="cuda")
        ci = torch.empty(n, dtype=torch.int32, device="cuda")
        cc = torch.zeros(1, dtype=torch.int32, device="cuda")
        vis = torch.zeros(n, dtype=torch.uint8, device="cuda")
        splat = torch.zeros((n, 4), dtype=torch.int64, device="cuda")

        def vertices(compact):
            def run():
                if compact:
                    cc.zero_()
                ctx.connect_vertices(eye, light, mat, pipe.min_t, eye_prev, light_prev, out=rec,
                                     compact=(cr, ci, cc) if compact else None, stream=sp)
            return run

        def camera(compact):
            def run():
                if compact:
                    cc.zero_()
                ctx.connect_camera(light, W, H, (0.5, 0.5), mat, pipe.min_t, out=cam, compact=(cr, ci, cc) if compact else None,
                                   stream=sp)
            return run

        rec_bytes = (4 if mat else 6) * 16
        for q, fn, status_of, bit in (("vertices", vertices(False), None, 1), ("vertices+compact", vertices(True), rec, 1),
                                      ("camera", camera(False), None, 2), ("camera+compact", camera(True), cam, 2)):
            ms = time_ms(torch, fn, st, args.warmup, args.reps)
            torch.cuda.synchronize()
            vert = q.startswith("vertices")
            by = (2 * rec_bytes + (0 if mat else 32) + 48) if vert else (rec_bytes + 64)
            line = {"mat": mat, "query": q, "n": n, "ms": round(ms, 4), "mitems_s": round(n / ms / 1e3, 1)}
            if status_of is not None:
                status = status_of.view(torch.int32)[:, 11 if vert else 13]
                worth = round(float(((status & bit) != 0).float().mean()), 4)
                by += 36 * worth
                line["rays_worth_tracing"] = worth
                line["trace_any_ms"] = round(time_ms(torch, lambda: ctx.trace_rays(cr, "any", out=vis, count=cc, stream=sp), st,
                                                     args.warmup, args.reps), 4)
            line.update({"bytes": round(by, 1), "gb_s": round(by * line["mitems_s"] / 1e3, 1)})
            emit(line)
        # the compact list of CAMERA mode and its visibility bytes are what the last iteration left
        torch.cuda.synchronize()
        k = int(cc.item())
        pixels = cam.view(torch.int32)[:, 12].contiguous()
        values = torch.cat([cam[:, 8:11] * cam[:, 11:12], torch.zeros((n, 1), device="cuda")], dim=1).clamp_(0.0, 0.9).contiguous()
        # every entry lands: the items without a pixel take their own index as the target (spread over the frame) ...
        every = torch.where(pixels < 0, torch.arange(n, dtype=torch.int32, device="cuda"), pixels)
        hot = pixels.clamp(min=0)  # ... or all pixel 0: the atomics of ~0.4 n entries on one 32-byte accumulator
        for q, fn, entries, by in (("splat_add", lambda: ctx.splat_add(splat, every, values, stream=sp), n, 20),
                                   ("splat_add hot pixel", lambda: ctx.splat_add(splat, hot, values, stream=sp), n, 20),
                                   ("splat_add+items", lambda: ctx.splat_add(splat, pixels, values, vis, ci, cc, stream=sp), k, 25)):
            ms = time_ms(torch, fn, st, args.warmup, args.reps)
            mis = entries / ms / 1e3
            emit({"mat": mat, "query": q, "n": entries, "ms": round(ms, 4), "mitems_s": round(mis, 1), "bytes": by,
                  "gb_s": round(by * mis / 1e3, 1), "visible": round(float((vis[:k] != 0).float().mean()), 4) if "items" in q else None})
        del rays, hits, eye, light, rec, cam, cr, ci, cc, vis, splat
        pipe.close()
    scene.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
