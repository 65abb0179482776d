"""The resampled direct lighting query (csrc/ris.hip) against what it replaces and what it estimates, one item per pixel at
1920x1080 on the bench scene (the 262 k-triangle atrium): the items are the G-buffer vertices (bdpt_shade_hits' records of the
primary hits), the lights the 16-light table of tools/direct_times.py.  One JSON line per measurement:

  fused      median device time of one Context.ris_lighting call (HIP events around it on its stream) for candidates M in
             1, 4, 8, 32 x samples K in 1, 8, both materials, without and with BDPT_PARAM_AREA_LIGHTS
  loop       the composed loop kept wholly on the device for K = 1, Lambertian: per candidate sample_lights(seeds_out=seeds) ->
             a draw, clamp, weight and reservoir update in torch on preallocated tensors, then one trace_rays("any") over the
             survivors' rays and an add; nothing returns to the host
  direct     Context.direct_lighting on the same table: the converged answer this estimates (16 rays an item)
  nee        sample_lights + trace_rays("any") for one sample: the M = 1 floor
  mse        at equal ray count (K = 8) the mean squared error of the fused estimate against direct_lighting's colour over the
             alive items whose diffuse colour is not near black (direct_lighting has a specular fallback there), for M = 1, 4, 8
             and 32, and its ratio to M = 1: the variance the resampling buys

The variants run --warmup times, then alternate --reps times in one process; medians, minima and maxima are over those
repetitions.  --fused-only times the fused calls alone: for comparing builds of the kernel (make -C csrc
EXTRA=-DBDPT_RIS_REGEN_MIN=16, -DBDPT_RIS_WAVES_PER_EU=3, its build knobs), one run per build.

  timeout 900 python tools/ris_times.py [--reps 20] [--fused-only] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

W, H = 1920, 1080
FLT_MAX = 3.4028234663852886e38


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=262144)
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lights", type=int, default=16)
    ap.add_argument("--fused-only", action="store_true", help="time the fused calls alone (comparing builds of the kernel)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as ge
    from direct_times import light_table
    pkg = ge.load_package()
    abi = pkg.abi
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

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
    lights = light_table(abi, args.lights, lo, hi)
    desc = abi.SceneDesc.from_buffer_copy(d0)
    desc.lights, desc.numLights = lights, args.lights
    ctx = pkg.Context(0)
    ctx.set_scene(desc)

    seeds0 = torch.from_numpy(np.random.default_rng(3).integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)).cuda()
    seeds = torch.empty(n, **i32)
    col, ref = torch.empty((n, 4), **f32), torch.empty((n, 4), **f32)
    ls, acc = torch.empty((n, 12), **f32), torch.empty((n, 3), **f32)
    ray_sel, v_sel = torch.empty((n, 8), **f32), torch.empty((n, 3), **f32)
    w_sel, wsum = torch.empty(n, **f32), torch.empty(n, **f32)
    vis = torch.empty(n, dtype=torch.uint8, device="cuda")

    def run_fused(M, K, mat=1, area=False, hints=False):
        ctx.ris_lighting(surf, seeds0, M, K, mat_index=mat, area_lights=area, use_hints=hints, min_t=min_t, out=col, stream=sp)

    def run_loop(M):
        seeds.copy_(seeds0)
        wsum.zero_()
        w_sel.zero_()
        v_sel.zero_()
        ray_sel.zero_()
        for _ in range(M):
            ctx.sample_lights(surf, seeds, mat_index=1, min_t=min_t, out=ls, seeds_out=seeds, stream=sp)
            seeds.mul_(1664525).add_(1013904223)
            u = (seeds & 0x00FFFFFF).float() / 16777216.0
            v = torch.where(ls[:, 8:11] > 0, ls[:, 8:11], torch.zeros((), **f32)).clamp(max=FLT_MAX)
            wc = v.max(dim=1).values
            wsum.add_(wc)
            take = (wc > 0) & (u * wsum <= wc)
            v_sel.copy_(torch.where(take[:, None], v, v_sel))
            w_sel.copy_(torch.where(take, wc, w_sel))
            ray_sel.copy_(torch.where(take[:, None], ls[:, 0:8], ray_sel))
        ctx.trace_rays(ray_sel, "any", out=vis, stream=sp)
        term = v_sel * ((wsum / float(M)) / w_sel)[:, None]
        acc.copy_(torch.where(((w_sel > 0) & (vis != 0) & live)[:, None], term, torch.zeros((), **f32)))

    def run_nee():
        ctx.sample_lights(surf, seeds0, mat_index=1, min_t=min_t, out=ls, stream=sp)
        ray_sel.copy_(ls[:, 0:8])
        ctx.trace_rays(ray_sel, "any", out=vis, stream=sp)

    def run_direct():
        ctx.direct_lighting(surf, min_t=min_t, out=ref, stream=sp)

    # the loop is the call: checked once, before timing (tests/test_gpu_ris.py has the bit-for-bit comparisons over the yardstick).
    # bits_equal: every colour word of every alive item; close: 1e-4 relative, the least that must hold before a time is
    # written down (torch's float division need not round as the kernel's does)
    equal, bits_equal = {}, {}
    for M in (1, 8):
        run_fused(M, 1)
        run_loop(M)
        torch.cuda.synchronize()
        ok = live & ~torch.isnan(acc).any(dim=1)
        equal[M] = bool(torch.allclose(col[ok][:, 0:3], acc[ok], rtol=1e-4, atol=1e-6))
        bits_equal[M] = bool(torch.equal(col[live][:, 0:3].contiguous().view(torch.int32), acc[live].contiguous().view(torch.int32)))
    emit({"n": n, "lights": args.lights, "alive": round(float(live.float().mean()), 4), "loop_equals_fused": equal,
          "loop_bits_equal_fused": bits_equal})
    if not all(equal.values()):
        sys.exit("ris_times: the composed loop and the fused call differ: no time is written down")

    variants = []
    for mat in (1, 0):
        for area in (False, True):
            for M in (1, 4, 8, 32):
                for K in (1, 8):
                    variants.append((f"fused_M{M}_K{K}_{'ggx' if mat == 0 else 'lambert'}{'_area' if area else ''}",
                                     lambda M=M, K=K, mat=mat, area=area: run_fused(M, K, mat, area)))
    variants.append(("fused_M8_K1_lambert_hints", lambda: run_fused(8, 1, 1, False, True)))
    if not args.fused_only:
        variants += [(f"loop_M{M}_K1_lambert", lambda M=M: run_loop(M)) for M in (1, 4, 8, 32)]
        variants += [("direct", run_direct), ("nee", run_nee)]
    for _ in range(args.warmup):
        for _, fn in variants:
            fn()
    ms = {k: [] for k, _ in variants}
    for _ in range(args.reps):
        for k, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    for k, _ in variants:
        emit({"variant": k, "ms": round(statistics.median(ms[k]), 3), "min_ms": round(min(ms[k]), 3), "max_ms": round(max(ms[k]), 3)})

    if not args.fused_only:
        run_direct()
        torch.cuda.synchronize()
        dif = surf[:, 12:15]
        both = live & ((dif * dif).sum(dim=1) >= 1e-4) & ~torch.isnan(ref[:, 0:3]).any(dim=1)
        want = ref[both][:, 0:3].double()
        base = None
        for M in (1, 4, 8, 32):
            run_fused(M, 8)
            torch.cuda.synchronize()
            mse = float(((col[both][:, 0:3].double() - want) ** 2).mean())
            base = mse if base is None else base
            emit({"mse_M": M, "K": 8, "mse": mse, "over_M1": round(mse / base, 4), "mean_ref": float(want.mean()),
                  "mean_est": float(col[both][:, 0:3].double().mean())})
    torch.cuda.synchronize()
    ctx.close()
    scene.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
