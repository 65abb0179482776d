"""Costs of motion (bdpt_keep_pose, bdpt_gbuffer_execute_motion, bdpt_bmfr_execute_motion) on the BASELINE shapes configs[2]
(atrium 262 k) and configs[4] (courtyard 10 M), 1920x1080.  One JSON line per shape, every time the median of device events
after warm-up; the calls of a comparison alternate in one process, the plain one being the entry point as it was before
there was motion (its kernel instances are unchanged):

  keep_pose_ms     bdpt_keep_pose alone; gbytes_per_s: the 96 B per primitive it moves (48 read of a 112-B shading record,
                   48 written) over that time, and its share of the 6.29 TB/s a float4 copy reaches
  gbuffer_ms       bdpt_gbuffer_execute / bdpt_gbuffer_execute_motion (pinhole, the pipeline's jitter)
  bmfr_ms          bdpt_bmfr_execute / bdpt_bmfr_execute_motion on the G-buffer of a moved scene (every vertex displaced, so
                   PrevWorldPosition differs from WorldPosition), with the camera's own view-projection as prevViewProj:
                   "pre_post" the default stages, "all" with the regression

  python tools/motion_times.py [--configs 2,4 | atrium:N,courtyard:N] [--reps 10] [--width 1920 --height 1080]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

HBM_COPY_TBS = 6.29


def view_proj_of(cam):
    """clip = M (p, 1) for the pinhole camera whose primary ray of NDC (x, y) is x U + y V + W: x = clip.x / clip.w"""
    pos = np.array(list(cam.posW), np.float64)
    m = np.zeros((4, 4))
    for row, axis in ((0, cam.cameraU), (1, cam.cameraV), (3, cam.cameraW)):
        a = np.array(list(axis), np.float64)
        a /= a @ a
        m[row, :3], m[row, 3] = a, -(pos @ a)
    return [float(x) for x in m.reshape(-1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,4")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    A = pkg.abi
    shapes = {"2": ("atrium 262k", lambda: pkg.Scene.atrium(1, 262144)),
              "4": ("courtyard 10M", lambda: pkg.Scene.courtyard(1, 10000000))}
    st = torch.cuda.current_stream()
    W, H = args.width, args.height

    def timed(fns):
        """median device ms of every callable of `fns`, the callables alternating within each repetition"""
        ms = [[] for _ in fns]
        for r in range(2 + args.reps):
            for k, fn in enumerate(fns):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                fn(r)
                e1.record(st)
                torch.cuda.synchronize()
                if r >= 2:
                    ms[k].append(e0.elapsed_time(e1))
        return [round(statistics.median(m), 4) for m in ms]

    for key in args.configs.split(","):
        if ":" in key:  # atrium:N / courtyard:N: the same scene at another triangle count
            kind, tris = key.split(":")
            name, make = f"{kind} {tris}", (lambda k=kind, t=int(tris): getattr(pkg.Scene, k)(1, t))
        else:
            name, make = shapes[key]
        scene = make()
        d = scene.desc
        nt = int(d.numTriangles)
        pipe = pkg.FramePipeline(scene, W, H, max_depth=3, motion=True)
        sp = pipe._stream_ptr()
        out = {"shape": name, "triangles": nt, "frame": [W, H]}
        keep = timed([lambda _: pipe.ctx.keep_pose(sp)])[0]
        gbs = nt * 96 / (keep * 1e-3) / 1e9
        out["keep_pose_ms"] = keep
        out["keep_pose_gbytes_per_s"] = round(gbs, 1)
        out["keep_pose_share_of_hbm_copy_rate"] = round(gbs / (HBM_COPY_TBS * 1e3), 3)
        # a moved scene: the previous pose stays the scene as loaded
        P = np.ctypeslib.as_array(d.positions, shape=(int(d.numVertices), 3)).astype(np.float32)
        ext = float(np.max(P.max(axis=0) - P.min(axis=0)))
        moved = P + np.float32(0.002 * ext) * np.sin(P[:, [1, 2, 0]] * np.float32(40.0 / ext))
        moved = torch.from_numpy(np.ascontiguousarray(moved, dtype=np.float32)).cuda()  # (the fancy index is not C-ordered)
        pipe.ctx.update_geometry(moved, stream=sp, keep_light_maps=True)
        gp = pipe.gbuffer_params()
        prev = C.c_void_p(pipe.prev_position.data_ptr())
        g = timed([lambda _: pipe.ctx.gbuffer_execute(gp, pipe.gb, sp), lambda _: pipe.ctx.gbuffer_execute_motion(gp, pipe.gb, prev, sp)])
        out["gbuffer_ms"] = {"plain": g[0], "motion": g[1]}
        torch.cuda.synchronize()
        differ = (pipe.prev_position[..., :3] != pipe.channels["WorldPosition"][..., :3]).any(dim=-1).float().mean().item()
        out["pixels_with_motion"] = round(differ, 3)
        noisy = torch.rand(H, W, 4, dtype=torch.float32, device=pipe.dev)
        noisy[..., 3] = 1.0
        work = noisy.clone()
        vp = view_proj_of(pipe.cam)
        out["bmfr_ms"] = {}
        for label, flags in (("pre_post", A.BMFR_PREPROCESS | A.BMFR_POSTPROCESS),
                             ("all", A.BMFR_PREPROCESS | A.BMFR_REGRESSION | A.BMFR_POSTPROCESS)):
            p = A.BmfrParams()
            p.frameNumber, p.flags = 1, flags
            for i in range(16):
                p.prevViewProj[i] = vp[i]

            def plain(_):
                pipe.ctx.bmfr_execute(p, pipe.gb, C.c_void_p(work.data_ptr()), sp)

            def motion(_):
                pipe.ctx.bmfr_execute_motion(p, pipe.gb, prev, C.c_void_p(work.data_ptr()), sp)

            work.copy_(noisy)
            b = timed([plain, motion])
            out["bmfr_ms"][label] = {"plain": b[0], "motion": b[1]}
        print(json.dumps(out), flush=True)
        pipe.close()
        scene.close()
        del moved, noisy, work
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
