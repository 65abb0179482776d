"""The reservoir reuse query (csrc/reuse.hip) against what it replaces and what it buys, one item per pixel at 1920x1080 on the
bench scene (the 262 k-triangle atrium): the items are the G-buffer vertices (bdpt_shade_hits' records of the primary hits), the
lights the 16-light table of tools/direct_times.py, the own and pool records those of one Context.ris_lighting call with 8
candidates, the neighbours pixels at offsets drawn within a radius of 8.  One JSON line per measurement:

  fused      median device time of one Context.reuse_lighting call (HIP events around it on its stream) for neighbors 1 and 4,
             both materials, without and with BDPT_PARAM_AREA_LIGHTS
  loop       the composed loop kept wholly on the device, Lambertian and GGX: per source the neighbour tests and gathers in
             torch, prev(state) -> sample_lights -> clamp, weight and reservoir update on preallocated tensors; per neighbour
             a gather of its record and sample_lights for Z; then one trace_rays("any") and the term; nothing returns to the host
  mse        at one ray per pixel and pass the mean squared error against Context.direct_lighting's colour over the alive items
             whose diffuse colour is not near black: ris_lighting with 8 candidates alone, with 4 spatial neighbours, with the
             same pixel's record of the frame before over 8 static frames, and with both; and ris_lighting with 32 candidates.
             The time of every pass of the last frame stands beside it.

The variants run --warmup times, then alternate --reps times in one process; medians, minima and maxima are over those
repetitions.  --fused-only times the fused calls alone: for comparing builds of the kernel (make -C csrc
EXTRA=-DBDPT_REUSE_REGEN_MIN=32, its build knob), one run per build.

  timeout 900 python tools/reuse_times.py [--reps 20] [--fused-only] [--out FILE]
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
M1 = 8  # the first stage's candidates


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=262144)
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lights", type=int, default=16)
    ap.add_argument("--radius", type=int, default=8)
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

    rng = np.random.default_rng(3)
    seeds0 = torch.from_numpy(rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)).cuda()
    seeds1 = torch.from_numpy(rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)).cuda()
    # neighbours: pixels at offsets drawn within the radius; outside the frame or the pixel itself: none
    x, y = np.arange(n) % w, np.arange(n) // w
    off = rng.integers(-args.radius, args.radius + 1, (n, 4, 2))
    nx, ny = x[:, None] + off[..., 0], y[:, None] + off[..., 1]
    ok = ((off != 0).any(axis=2)) & (nx >= 0) & (ny >= 0) & (nx < w) & (ny < h)
    nbr4 = torch.from_numpy(np.where(ok, ny * w + nx, -1).astype(np.int32)).cuda()
    nbr = {1: nbr4[:, :1].contiguous(), 4: nbr4}
    same = torch.arange(n, **i32)[:, None].contiguous()
    col, ref = torch.empty((n, 4), **f32), torch.empty((n, 4), **f32)
    first = {}
    for mat, area in ((1, False), (0, False), (1, True), (0, True)):
        r = torch.empty((n, 1, 4), **i32)
        ctx.ris_lighting(surf, seeds1, M1, 1, mat_index=mat, area_lights=area, min_t=min_t, out=col, reservoirs=r, stream=sp)
        first[(mat, area)] = r.view(n, 4)
    res_out = torch.empty((n, 4), **i32)
    reject = dict(normal_min=0.9, plane_max=float("inf"))

    def run_fused(K, mat=1, area=False):
        ctx.reuse_lighting(surf, seeds0, first[(mat, area)], neighbor_index=nbr[K] if K else None, in_m=M1, pool_m=M1, mat_index=mat,
                           area_lights=area, min_t=min_t, out=col, reservoirs_out=res_out, stream=sp, **reject)

    # ---- the composed loop, on preallocated tensors ----
    seeds, prev = torch.empty(n, **i32), torch.empty(n, **i32)
    ls, acc = torch.empty((n, 12), **f32), torch.empty((n, 3), **f32)
    ray_sel, v_sel = torch.empty((n, 8), **f32), torch.empty((n, 3), **f32)
    t_sel, wsum = torch.empty(n, **f32), torch.empty(n, **f32)
    state_sel, Z = torch.empty(n, **i32), torch.empty(n, **i32)
    vis = torch.empty(n, dtype=torch.uint8, device="cuda")
    zero = torch.zeros((), **f32)
    pos, nrm = surf[:, 0:3], surf[:, 4:7]

    def dot(a, b):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]

    def value_at(records, states, mat):
        prev.copy_(states)
        prev.sub_(1013904223).mul_(4276115653 - 2**32)  # the generator's inverse, mod 2^32
        ctx.sample_lights(records, prev, mat_index=mat, min_t=min_t, out=ls, stream=sp)
        v = torch.where(ls[:, 8:11] > 0, ls[:, 8:11], zero).clamp(max=FLT_MAX)
        return v, v.max(dim=1).values

    def run_loop(K, mat=1):
        res = first[(mat, False)]
        seeds.copy_(seeds0)
        for t in (wsum, t_sel, v_sel, ray_sel):
            t.zero_()
        state_sel.zero_()
        used = []
        for j in range(K + 1):
            seeds.mul_(1664525).add_(1013904223)
            u = (seeds & 0x00FFFFFF).float() / 16777216.0
            if j == 0:
                okj, y = live, res
            else:
                p = nbr[K][:, j - 1]
                q = p.clamp(min=0).long()
                okj = live & (p >= 0) & live[q] & (dot(nrm, nrm[q]) >= reject["normal_min"]) & \
                    (dot(nrm, pos[q] - pos).abs() <= reject["plane_max"])
                y = res[q]
                used.append((okj, q))
            Wy = y[:, 2].view(torch.float32)
            full = okj & ((y[:, 0] & 0xFFFF) < args.lights) & (Wy > 0)
            v, t = value_at(surf, y[:, 1], mat)
            wj = torch.where(full, (t * Wy) * float(M1), zero)
            wsum.add_(wj)
            take = (wj > 0) & (u * wsum <= wj)
            v_sel.copy_(torch.where(take[:, None], v, v_sel))
            t_sel.copy_(torch.where(take, t, t_sel))
            ray_sel.copy_(torch.where(take[:, None], ls[:, 0:8], ray_sel))
            state_sel.copy_(torch.where(take, y[:, 1], state_sel))
        Z.copy_(torch.where(t_sel > 0, M1, 0))
        for okj, q in used:
            _, t = value_at(surf[q], state_sel, mat)
            Z.add_(torch.where(okj & (t_sel > 0) & (t > 0), M1, 0))
        ctx.trace_rays(ray_sel, "any", out=vis, stream=sp)
        term = v_sel * ((wsum / Z.float()) / t_sel)[:, None]
        acc.copy_(torch.where(((t_sel > 0) & (Z > 0) & (vis != 0) & live)[:, None], term, zero))

    # the loop is the call: checked once, before timing (tests/test_gpu_reuse.py has the bit-for-bit comparisons over the
    # yardstick).  close: 1e-4 relative, the least that must hold before a time is written down (torch's float division need
    # not round as the kernel's does); bits_equal: every colour word of every alive item
    equal, bits_equal = {}, {}
    if not args.fused_only:
        for K, mat in ((1, 1), (4, 1), (4, 0)):
            run_fused(K, mat)
            run_loop(K, mat)
            torch.cuda.synchronize()
            okc = live & ~torch.isnan(acc).any(dim=1) & ~torch.isnan(col[:, 0:3]).any(dim=1)
            equal[f"{K}_{mat}"] = bool(torch.allclose(col[okc][:, 0:3], acc[okc], rtol=1e-4, atol=1e-6))
            bits_equal[f"{K}_{mat}"] = bool(torch.equal(col[live][:, 0:3].contiguous().view(torch.int32), acc[live].contiguous().view(torch.int32)))
        emit({"n": n, "lights": args.lights, "alive": round(float(live.float().mean()), 4), "loop_equals_fused": equal,
              "loop_bits_equal_fused": bits_equal})
        if not all(equal.values()):
            sys.exit("reuse_times: the composed loop and the fused call differ: no time is written down")

    variants = []
    for mat in (1, 0):
        for area in (False, True):
            for K in (1, 4):
                variants.append((f"fused_N{K}_{'ggx' if mat == 0 else 'lambert'}{'_area' if area else ''}",
                                 lambda K=K, mat=mat, area=area: run_fused(K, mat, area)))
    if not args.fused_only:
        variants += [(f"loop_N{K}_{'ggx' if mat == 0 else 'lambert'}", lambda K=K, mat=mat: run_loop(K, mat)) for mat in (1, 0) for K in (1, 4)]
    for _ in range(args.warmup):
        for _, fn in variants:
            fn()
    ms = {k: [] for k, _ in variants}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(args.reps):
        for k, fn in variants:
            ms[k].append(timed(fn))
    for k, _ in variants:
        emit({"variant": k, "ms": round(statistics.median(ms[k]), 3), "min_ms": round(min(ms[k]), 3), "max_ms": round(max(ms[k]), 3)})

    if not args.fused_only:
        ctx.direct_lighting(surf, min_t=min_t, out=ref, stream=sp)
        torch.cuda.synchronize()
        dif = surf[:, 12:15]
        both = live & ((dif * dif).sum(dim=1) >= 1e-4) & ~torch.isnan(ref[:, 0:3]).any(dim=1)
        want = ref[both][:, 0:3].double()
        r1, a, b, hist = (torch.zeros((n, 4), **i32) for _ in range(4))

        def frames(spatial, temporal, count):
            """`count` static frames of RIS with M1 candidates and the chosen reuse passes -> the passes' times of the last"""
            times = {}
            for f in range(count):
                sd = seeds0 * (2 * f + 3) + f
                times["ris"] = timed(lambda: ctx.ris_lighting(surf, sd, M1, 1, min_t=min_t, out=col, reservoirs=r1.view(n, 1, 4), stream=sp))
                cur, in_m = r1, M1
                if temporal and f:
                    times["temporal"] = timed(lambda: ctx.reuse_lighting(
                        surf, sd + 77, cur, neighbor_index=same, pool_surfaces=surf, pool_reservoirs=hist, in_m=in_m, max_m=20 * M1,
                        min_t=min_t, out=col, reservoirs_out=a, stream=sp, **reject))
                    cur, in_m = a, 0
                if spatial:
                    times["spatial"] = timed(lambda: ctx.reuse_lighting(
                        surf, sd + 99, cur, neighbor_index=nbr[4], in_m=in_m, pool_m=in_m, max_m=20 * M1, min_t=min_t, out=col,
                        reservoirs_out=b, stream=sp, **reject))
                    cur, in_m = b, 0
                hist.copy_(cur)
                if in_m:
                    hist[:, 3] = in_m
            return times

        for name, spatial, temporal, count in (("ris8", False, False, 1), ("ris8_spatial4", True, False, 1),
                                               ("ris8_temporal_8_frames", False, True, 8), ("ris8_both_8_frames", True, True, 8)):
            times = frames(spatial, temporal, count)
            torch.cuda.synchronize()
            mse = float(((col[both][:, 0:3].double() - want) ** 2).mean())
            emit({"mse_of": name, "mse": mse, "mean_ref": float(want.mean()), "mean_est": float(col[both][:, 0:3].double().mean()),
                  "pass_ms": {k: round(v, 3) for k, v in times.items()}, "frame_ms": round(sum(times.values()), 3)})
        t32 = timed(lambda: ctx.ris_lighting(surf, seeds0, 32, 1, min_t=min_t, out=col, stream=sp))
        torch.cuda.synchronize()
        emit({"mse_of": "ris32", "mse": float(((col[both][:, 0:3].double() - want) ** 2).mean()), "frame_ms": round(t32, 3)})
    torch.cuda.synchronize()
    ctx.close()
    scene.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
