"""The sky lighting query (csrc/sky.hip) against the composed loop it replaces and against ambient occlusion, one item per
pixel at 1920x1080 on the bench scene (the 262 k-triangle atrium): the items are the G-buffer vertices (bdpt_shade_hits'
records of the primary hits), the environment is a procedural 2048x1024 sky with a sun.  One JSON line per sample count S
(default 1, 8, 32):

  fused_ms   median device time of one Context.sky_lighting call (HIP events around it on its stream)
  loop_ms    median device time of the composed loop on the same inputs, wholly on the device and into preallocated
             tensors: per sample env_sample(Lambertian, seeds advanced in place) -> the clamp -> trace_rays(any) on every
             item's ray -> one masked add, on one stream; nothing returns to the host
  ao_ms      median device time of Context.ambient_occlusion with the same S and an unbounded radius: as many any-hit
             rays per item without the table searches — the floor.  ao.hip's device code is the parent commit's (its
             listing is compared when the kernels change); --ao-only --root DIR times the same call in another checkout
             (a build of the parent commit), in a process of its own
  ratio      loop_ms / fused_ms;  over_ao = fused_ms / ao_ms
  traced     share of the alive items' samples that are worth a ray; unoccluded: share of those that reach the sky
  equal      fused and loop give the same colour words, counts and final states (checked once, before timing)

and one line per map size (default 2048x1024, 8192x4096) with prepare_ms, the median device time of bdpt_env_prepare on a
prepared context (three kernels), and the table's bytes.

The variants run --warmup times, then alternate --reps times in one process; the medians are over those repetitions, with
minimum and maximum beside them.  --fused-only times the fused call alone: for comparing builds of the kernel
(make -C csrc EXTRA=-DBDPT_SKY_WAVES_PER_EU=5), one run per build.

  timeout 900 python tools/sky_times.py [--samples 1,8,32] [--reps 20] [--fused-only] [--ao-only [--root DIR]] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H = 1920, 1080
FLT_MAX = 3.4028234663852886e38


def sky_map(torch, w, h):
    """a blue gradient above a dark ground, with a sun of 3 x 3 texels at 1e5"""
    v = (torch.arange(h, device="cuda", dtype=torch.float32) + 0.5) / h
    up = torch.clamp(1.0 - 2.0 * v, min=0.0)[:, None].expand(h, w)
    env = torch.ones((h, w, 4), dtype=torch.float32, device="cuda")
    env[..., 0], env[..., 1], env[..., 2] = 0.05 + 0.3 * up, 0.05 + 0.5 * up, 0.05 + 0.9 * up
    env[h // 5 - 1:h // 5 + 2, w // 3 - 1:w // 3 + 2, 0:3] = 1e5
    return env.contiguous()


def timed(torch, st, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=262144)
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--samples", default="1,8,32")
    ap.add_argument("--maps", default="2048x1024,8192x4096")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fused-only", action="store_true", help="time the fused call alone (comparing builds of the kernel)")
    ap.add_argument("--ao-only", action="store_true", help="time bdpt_ao_query alone: needs no environment entry point")
    ap.add_argument("--root", default=None, help="the checkout whose package is loaded (default: this one)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    if args.root:
        sys.path.insert(0, os.path.abspath(args.root))
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
    rays0 = ctx.camera_rays(pipe.gbuffer_params(), w, h, stream=sp)
    hits = torch.empty((n, 4), **f32)
    ctx.trace_rays(rays0, "closest_cull_back", out=hits, stream=sp)
    surf = ctx.shade_hits(rays0, hits, True, stream=sp)
    seeds = torch.arange(n, **i32) * 1103515245
    live = surf.view(torch.int32)[:, 23] >= 0
    del rays0, hits

    if args.ao_only:
        for S in [int(x) for x in args.samples.split(",")]:
            ao, ao_counts, ao_sout = torch.empty(n, **f32), torch.empty(n, **i32), torch.empty(n, **i32)

            def run_ao():
                ctx.ambient_occlusion(surf, seeds, S, float("inf"), min_t=pipe.min_t, out=ao, counts=ao_counts, seeds_out=ao_sout, stream=sp)

            for _ in range(args.warmup):
                run_ao()
            ms = [timed(torch, st, run_ao) for _ in range(args.reps)]
            line = {"n": n, "samples": S, "ao_ms": round(statistics.median(ms), 3), "ao_min_ms": round(min(ms), 3),
                    "ao_max_ms": round(max(ms), 3), "package": os.path.dirname(os.path.abspath(ge.__file__))}
            print(json.dumps(line), flush=True)
            lines.append(line)
        pipe.close()
        scene.close()
        if args.out:
            with open(args.out, "w") as f:
                f.write("".join(json.dumps(l) + "\n" for l in lines))
        return

    # the table: once per map size, re-prepared in place for the timing
    for size in [s for s in args.maps.split(",") if s]:
        mw, mh = (int(x) for x in size.split("x"))
        env = sky_map(torch, mw, mh)
        ctx.set_environment(env.data_ptr(), mw, mh)
        ctx.env_prepare(sp)
        torch.cuda.synchronize()
        for _ in range(args.warmup):
            ctx.env_prepare(sp)
        ms = [timed(torch, st, lambda: ctx.env_prepare(sp)) for _ in range(args.reps)]
        info = ctx.env_info()
        line = {"map": size, "prepare_ms": round(statistics.median(ms), 3), "prepare_min_ms": round(min(ms), 3),
                "prepare_max_ms": round(max(ms), 3), "table_bytes": int(info.tableBytes), "total": int(info.total)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        ctx.set_environment()
        del env

    env = sky_map(torch, 2048, 1024)
    ctx.set_environment(env.data_ptr(), 2048, 1024)
    ctx.env_prepare(sp)
    hi = torch.tensor(FLT_MAX, **f32)
    zero = torch.zeros((), **f32)
    for S in [int(x) for x in args.samples.split(",")]:
        col, counts, sout = torch.empty((n, 4), **f32), torch.empty(n, **i32), torch.empty(n, **i32)
        ao, ao_counts, ao_sout = torch.empty(n, **f32), torch.empty(n, **i32), torch.empty(n, **i32)
        smp, vis = torch.empty((n, 20), **f32), torch.empty(n, dtype=torch.uint8, device="cuda")
        rays = torch.empty((n, 8), **f32)
        loop = {"sum": torch.empty((n, 3), **f32), "counts": torch.empty(n, **i32), "sout": torch.empty(n, **i32),
                "col": torch.ones((n, 4), **f32), "traced": torch.zeros((), dtype=torch.int64, device="cuda")}

        def run_fused():
            ctx.sky_lighting(surf, seeds, S, min_t=pipe.min_t, out=col, counts=counts, seeds_out=sout, stream=sp)

        def run_loop(tally=False):
            s, cnt, total = loop["sout"], loop["counts"], loop["sum"]
            s.copy_(seeds)
            cnt.zero_()
            total.zero_()
            for _ in range(S):
                ctx.env_sample(surf, s, mat_index=1, min_t=pipe.min_t, out=smp, seeds_out=s, stream=sp)  # (a miss record: a zero sample)
                v = smp[:, 12:15]
                value = torch.minimum(torch.where(v > 0, v, zero), hi)  # clampVec (no NaN survives the first step)
                rays.copy_(smp[:, 0:8])
                ctx.trace_rays(rays, "any", out=vis, stream=sp)
                worth = (value != 0).any(dim=1) & live
                add = worth & (vis != 0)
                total.add_(torch.where(add[:, None], value, zero))
                cnt.add_(add)
                if tally:
                    loop["traced"] += worth.sum()
            # a dead item takes no draw in the query; env_sample advanced its state: put it back
            s.copy_(torch.where(live, s, seeds))
            loop["col"][:, 0:3] = torch.where(live[:, None], total / float(S), surf[:, 12:15])

        def run_ao():
            ctx.ambient_occlusion(surf, seeds, S, float("inf"), min_t=pipe.min_t, out=ao, counts=ao_counts, seeds_out=ao_sout, stream=sp)

        run_fused()
        run_loop(tally=True)
        torch.cuda.synchronize()
        equal = bool(torch.equal(col.view(torch.int32), loop["col"].view(torch.int32)) and torch.equal(counts, loop["counts"]) and
                     torch.equal(sout, loop["sout"]))
        traced = int(loop["traced"])
        variants = (("fused", run_fused), ("loop", run_loop), ("ao", run_ao))[:1 if args.fused_only else 3]
        for _ in range(args.warmup):
            for _, fn in variants:
                fn()
        ms = {k: [] for k, _ in variants}
        for _ in range(args.reps):
            for name, fn in variants:
                ms[name].append(timed(torch, st, fn))
        med = {k: statistics.median(v) for k, v in ms.items()}
        alive = int(live.sum())
        line = {"n": n, "samples": S, "fused_ms": round(med["fused"], 3), "fused_min_ms": round(min(ms["fused"]), 3),
                "fused_max_ms": round(max(ms["fused"]), 3), "equal": equal, "alive": round(alive / n, 4),
                "traced": round(traced / max(1, alive * S), 4), "unoccluded": round(float(counts[live].sum()) / max(1, traced), 4)}
        if not args.fused_only:
            line.update({"loop_ms": round(med["loop"], 3), "loop_min_ms": round(min(ms["loop"]), 3), "loop_max_ms": round(max(ms["loop"]), 3),
                         "ao_ms": round(med["ao"], 3), "ao_min_ms": round(min(ms["ao"]), 3), "ao_max_ms": round(max(ms["ao"]), 3),
                         "ratio": round(med["loop"] / med["fused"], 2), "over_ao": round(med["fused"] / med["ao"], 2)})
        print(json.dumps(line), flush=True)
        lines.append(line)
        del col, counts, sout, ao, ao_counts, ao_sout, smp, vis, rays, loop
    ctx.set_environment()
    pipe.close()
    scene.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
