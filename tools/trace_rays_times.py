"""Throughput of bdpt_trace_rays (csrc/trace_rays.hip) in Mrays/s, per scene, ray set and mode.  One JSON line each:

  scene     the 262 k-triangle atrium, the 262 k-triangle courtyard with alpha-masked foliage
  rays      camera   1920x1080 primary rays through the scene's camera (coherent)
            random   4 M incoherent rays: origins uniform in the scene's box, directions uniform, unbounded
            shadow   G-buffer-to-light segments: every pixel of a 1920x1080 G-buffer with geometry to a point light of the
                     scene (direction = light - position, not unit length; tmin 1e-4, tmax 0.999)
  mode      closest, closest_cull_back, any
  ms        median device time of one call (HIP events around it on its stream) after --warmup calls
  mrays_s   rays / ms / 1000

--with-test-trace also sends the same rays once through bdpt_test_trace (one lane per ray: test_trace_kernel), so that a
run under `rocprofv3 --kernel-trace --stats` lists both kernels' times on identical input.

  python tools/trace_rays_times.py [--scenes atrium,courtyard] [--sets camera,random,shadow] [--reps 10] [--with-test-trace]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODES = ("closest", "closest_cull_back", "any")
W, H = 1920, 1080


def camera_rays(cam):
    u, v, w, p = (np.array(a, np.float32) for a in (cam.cameraU, cam.cameraV, cam.cameraW, cam.posW))
    x, y = np.meshgrid((np.arange(W) + 0.5) / W * 2 - 1, (np.arange(H) + 0.5) / H * 2 - 1)
    d = w[None] + x.reshape(-1, 1) * u[None] - y.reshape(-1, 1) * v[None]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    n = d.shape[0]
    return np.concatenate([np.broadcast_to(p, (n, 3)), np.zeros((n, 1)), d, np.full((n, 1), 1e38)], axis=1).astype(np.float32)


def random_rays(desc, n, seed=1):
    rng = np.random.default_rng(seed)
    pos = np.ctypeslib.as_array(desc.positions, shape=(desc.numVertices, 3))
    o = rng.uniform(pos.min(axis=0), pos.max(axis=0), (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, np.zeros((n, 1)), d, np.full((n, 1), 1e38)], axis=1).astype(np.float32)


def shadow_rays(pipe, desc):
    import torch
    pipe.ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, pipe._stream_ptr())
    torch.cuda.synchronize()
    pos = pipe.channels["WorldPosition"].cpu().numpy().reshape(-1, 4)[:, :3]
    nrm = pipe.channels["WorldNormal"].float().cpu().numpy().reshape(-1, 4)[:, :3]
    ok = (np.linalg.norm(nrm, axis=1) > 0.5) & np.isfinite(pos).all(axis=1)
    lights = [desc.lights[i] for i in range(desc.numLights)]
    pts = np.array([l.posW[:] for l in lights if l.type != 1], np.float32)  # point / spot lights
    if not len(pts):
        return None
    p = pos[ok]
    lp = pts[np.arange(len(p)) % len(pts)]
    n = len(p)
    return np.concatenate([p, np.full((n, 1), 1e-4), lp - p, np.full((n, 1), 0.999)], axis=1).astype(np.float32)


def time_call(torch, ctx, rays, mode, out, st, warmup, reps):
    for _ in range(warmup):
        ctx.trace_rays(rays, mode, out=out, stream=C.c_void_p(st.cuda_stream))
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        ctx.trace_rays(rays, mode, out=out, stream=C.c_void_p(st.cuda_stream))
        e1.record(st)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="atrium,courtyard")
    ap.add_argument("--sets", default="camera,random,shadow")
    ap.add_argument("--random-rays", type=int, default=4 << 20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--with-test-trace", action="store_true")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    makers = {"atrium": lambda: pkg.Scene.atrium(1, 262144), "courtyard": lambda: pkg.Scene.courtyard(1, 262144)}
    lines = []
    for name in args.scenes.split(","):
        scene = makers[name]()
        pipe = pkg.FramePipeline(scene, W, H, max_depth=3)
        st = torch.cuda.current_stream()
        sets = {}
        for s in args.sets.split(","):
            r = {"camera": lambda: camera_rays(pipe.cam), "random": lambda: random_rays(scene.desc, args.random_rays),
                 "shadow": lambda: shadow_rays(pipe, scene.desc)}[s]()
            if r is not None:
                sets[s] = r
        for s, rays in sets.items():
            n = rays.shape[0]
            rt = torch.from_numpy(rays).cuda()
            hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
            vis = torch.empty((n,), dtype=torch.uint8, device="cuda")
            for mode in MODES:
                ms = time_call(torch, pipe.ctx, rt, mode, vis if mode == "any" else hits, st, args.warmup, args.reps)
                line = {"scene": name, "rays": s, "n": n, "mode": mode, "ms": round(ms, 4), "mrays_s": round(n / ms / 1e3, 1)}
                if mode == "any":
                    line["unoccluded"] = round(float(vis.float().mean()), 4)
                else:
                    line["hit"] = round(float((hits.view(torch.int32)[:, 3] >= 0).float().mean()), 4)
                if args.with_test_trace:  # the test hook's layout: org, dir, tmin, tmax
                    pipe.ctx.test_trace(rays[:, [0, 1, 2, 4, 5, 6, 3, 7]], MODES.index(mode))
                print(json.dumps(line), flush=True)
                lines.append(line)
            del rt, hits, vis
        pipe.close()
        scene.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
