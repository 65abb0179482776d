"""Cost of light groups (bdpt_execute_light_groups) on the bench frame: the 262 k-triangle atrium (three lights) at
1920x1080, depth 8, GGX.  The G-buffer is rendered once; then bdpt_execute and bdpt_execute_light_groups run alternately
on it, --reps times each after --warmup, timed by torch.cuda events around each call on its stream.  One JSON line:

  plain_ms / groups_ms   median device time of one call
  extra_ms, extra_pct    groups_ms - plain_ms, and that over plain_ms
  plane_mb, splat_mb     the planes written (numLights + 1 RGBA32F) and the per-light splat planes cleared every frame

  python tools/light_groups_times.py [--reps 20] [--warmup 3]
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
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    scene = pkg.Scene.atrium(1, 262144)
    K = int(scene.desc.numLights)
    pipe = pkg.FramePipeline(scene, W, H, max_depth=D, mat_index=0)
    pipe.ctx.prepare(pkg.abi.PREPARE_LIGHT_GROUPS)
    groups = torch.zeros(K + 1, H, W, 4, dtype=torch.float32, device=pipe.dev)
    st = pipe._stream_ptr()
    pipe.ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, st)
    p = pipe.bdpt_params()
    out = C.c_void_p(pipe.output.data_ptr())
    calls = {"plain": lambda: pipe.ctx.execute(p, pipe.gb, out, st),
             "groups": lambda: pipe.ctx.execute_light_groups(p, pipe.gb, out, C.c_void_p(groups.data_ptr()), st)}
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
    plain, grp = statistics.median(times["plain"]), statistics.median(times["groups"])
    print(json.dumps({"scene": "atrium", "width": W, "height": H, "depth": D, "lights": K, "reps": a.reps,
                      "plain_ms": round(plain, 3), "groups_ms": round(grp, 3), "extra_ms": round(grp - plain, 3),
                      "extra_pct": round(100.0 * (grp - plain) / plain, 2),
                      "plain_ms_minmax": [round(min(times["plain"]), 3), round(max(times["plain"]), 3)],
                      "groups_ms_minmax": [round(min(times["groups"]), 3), round(max(times["groups"]), 3)],
                      "plane_mb": round((K + 1) * W * H * 16 / 1e6, 1), "splat_mb": round(K * W * H * 32 / 1e6, 1)}))
    pipe.close()
    scene.close()


if __name__ == "__main__":
    main()
