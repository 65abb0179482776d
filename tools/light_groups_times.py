"""Cost of light groups on the bench frame: the 262 k-triangle atrium (three lights) at 1920x1080, depth 8, GGX.  The
G-buffer is rendered once; then bdpt_execute, bdpt_execute_light_groups and bdpt_execute_grouped at 1, 2 and K groups (K
= one group per light, the identity assignment) run alternately on it, --reps times each after --warmup, timed by
torch.cuda events around each call on its stream.  One JSON line:

  plain_ms / groups_ms    median device time of one bdpt_execute / bdpt_execute_light_groups call
  grouped_ms              {groups: median ms} of bdpt_execute_grouped (1: every light in one group, 2: light i in group
                          i % 2, K: the identity)
  extra_ms, extra_pct     groups_ms - plain_ms, and that over plain_ms; grouped_extra_ms the same per group count
  *_minmax                fastest and slowest call
  plane_mb, splat_mb      the planes written (numLights + 1 RGBA32F) and the per-light splat planes cleared every frame
                          by bdpt_execute_light_groups

--area-lights runs every call that takes it with BDPT_PARAM_AREA_LIGHTS (the atrium's lamp bodies are its emitters):
bdpt_execute and bdpt_execute_grouped at 1, 2 and K + 1 groups (the table in a group of its own); bdpt_execute_light_groups
refuses the switch and is left out.

  python tools/light_groups_times.py [--reps 20] [--warmup 3] [--area-lights]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H, D = 1920, 1080, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--area-lights", action="store_true")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    scene = pkg.Scene.atrium(1, 262144)
    K = int(scene.desc.numLights)
    area = pkg.abi.PARAM_AREA_LIGHTS if a.area_lights else 0
    n_src = K + (1 if area else 0)  # sources an assignment names
    pipe = pkg.FramePipeline(scene, W, H, max_depth=D, mat_index=0, flags=area)
    pipe.ctx.prepare(pkg.abi.PREPARE_LIGHT_GROUP_TABLE | (pkg.abi.PREPARE_AREA_LIGHTS if area else 0))
    groups = torch.zeros(n_src + 1, H, W, 4, dtype=torch.float32, device=pipe.dev)
    st = pipe._stream_ptr()
    pipe.ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, st)
    p = pipe.bdpt_params()
    out, gptr = C.c_void_p(pipe.output.data_ptr()), C.c_void_p(groups.data_ptr())
    calls = {"plain": lambda: pipe.ctx.execute(p, pipe.gb, out, st)}
    if not area:
        calls["groups"] = lambda: pipe.ctx.execute_light_groups(p, pipe.gb, out, gptr, st)
    counts = sorted({1, min(2, n_src), n_src})
    for n in counts:
        assignment = [i % n for i in range(n_src)]
        calls[f"grouped{n}"] = lambda assignment=assignment, n=n: pipe.ctx.execute_grouped(p, pipe.gb, out, gptr, assignment, n, st)
    times = {k: [] for k in calls}
    for i in range(a.warmup + a.reps):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in times.items()}
    plain = med["plain"]
    res = {"scene": "atrium", "width": W, "height": H, "depth": D, "lights": K, "area_lights": bool(area), "reps": a.reps,
           "plain_ms": round(plain, 3), "plain_ms_minmax": [round(min(times["plain"]), 3), round(max(times["plain"]), 3)]}
    if "groups" in med:
        grp = med["groups"]
        res.update({"groups_ms": round(grp, 3), "extra_ms": round(grp - plain, 3), "extra_pct": round(100.0 * (grp - plain) / plain, 2),
                    "groups_ms_minmax": [round(min(times["groups"]), 3), round(max(times["groups"]), 3)]})
    res["grouped_ms"] = {str(n): round(med[f"grouped{n}"], 3) for n in counts}
    res["grouped_extra_ms"] = {str(n): round(med[f"grouped{n}"] - plain, 3) for n in counts}
    res["grouped_ms_minmax"] = {str(n): [round(min(times[f"grouped{n}"]), 3), round(max(times[f"grouped{n}"]), 3)] for n in counts}
    res["grouped_mb"] = {str(n): round(((n + 1) * 16 + n * 32) * W * H / 1e6, 1) for n in counts}  # planes written + splat planes cleared
    if area:
        res["emitters"] = int(pipe.ctx.area_light_info().numEmitters)
    res.update({"plane_mb": round((K + 1) * W * H * 16 / 1e6, 1), "splat_mb": round(K * W * H * 32 / 1e6, 1)})
    print(json.dumps(res))
    pipe.close()
    scene.close()


if __name__ == "__main__":
    main()
