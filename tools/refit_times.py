"""Costs of animated scenes (bdpt_update_geometry / bdpt_set_scene) on the BASELINE shapes configs[2] (atrium 262 k,
1920x1080, depth 8) and configs[4] (courtyard 10 M, 3840x2160, depth 16).  One JSON line per shape:

  update_ms        bdpt_update_geometry, device events around the call on the frame's stream, median after warm-up:
                   device / host pointers x light maps re-traced / kept (BDPT_UPDATE_KEEP_LIGHT_MAPS); host-pointer
                   updates also with their wall time (finiteness check + pinned copy happen before the call returns)
  set_scene_s      bdpt_set_scene of the swayed scene (wall, synchronised)
  trees            frame ms (median) and per-ray node visits / triangle tests / alpha tests (BDPT_PARAM_COUNTERS) for the
                   tree as built, after the sway (30 updates, light maps kept), and after a rebuild of the swayed scene;
                   hintedNee of each
  sah_ratio        sahCost / sahCostBuilt after the sway

The sway: a small smooth displacement (0.5 % of the scene extent at most) of the foliage vertices (those of alpha-mode
materials; in a scene without any, its upper half) over 30 frames, ending where it started.

With --pieces, in the same run, the piece-tight refit (bdpt_prepare(BDPT_PREPARE_REFIT_PIECES)) on the rebuilt tree:

  pieces.prepare_ms / table_bytes   the prepare after BDPT_PREPARE_REFIT (wall, synchronised: the regions alone) and the
                                    region table (24 B per record)
  pieces.update_ms                  device-pointer updates, light maps re-traced / kept, as update_ms above (the plain
                                    figures to compare with are update_ms.device_* of the same line)
  pieces.sah_ratio, trees.after_sway_pieces
                                    the same 30-update sway as above, refitted by pieces

  python tools/refit_times.py [--configs 2,4] [--frames 5] [--pieces]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,4")
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pieces", action="store_true")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    shapes = {"2": ("atrium 262k 1920x1080 d8", lambda: pkg.Scene.atrium(1, 262144), 1920, 1080, 8),
              "4": ("courtyard 10M 3840x2160 d16", lambda: pkg.Scene.courtyard(1, 10000000), 3840, 2160, 16)}
    for key in args.configs.split(","):
        name, make, W, H, D = shapes[key]
        scene = make()
        d = scene.desc
        p0 = np.ctypeslib.as_array(d.positions, shape=(d.numVertices, 3)).copy()
        idx = np.ctypeslib.as_array(d.indices, shape=(d.numTriangles, 3))
        mats = np.ctypeslib.as_array(d.triMaterial, shape=(d.numTriangles,))
        alpha_mat = np.array([(d.materials[m].flags >> 17) & 3 for m in range(d.numMaterials)]) != 0
        sway = np.zeros(d.numVertices, bool)
        sway[idx[alpha_mat[mats]].reshape(-1)] = True
        if not sway.any():
            sway = p0[:, 1] > np.median(p0[:, 1])
        ext = float(np.max(p0.max(axis=0) - p0.min(axis=0)))
        sw = p0[sway].astype(np.float64)

        def pose(t):
            p = p0.copy()
            a = 0.005 * ext * np.sin(2 * np.pi * t / 30.0)
            p[sway, 0] = (sw[:, 0] + a * np.sin(sw[:, 1] * (6.0 / ext))).astype(np.float32)
            p[sway, 2] = (sw[:, 2] + 0.5 * a * np.cos(sw[:, 1] * (4.0 / ext))).astype(np.float32)
            return p

        pipe = pkg.FramePipeline(scene, W, H, max_depth=D, mat_index=0)
        st = torch.cuda.current_stream()

        def frames():
            pipe.render_frame()
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.frames):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                pipe.render_frame()
                e1.record(st)
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            pipe.render_frame(extra_flags=pkg.abi.PARAM_COUNTERS)
            torch.cuda.synchronize()
            c = pipe.ctx.counters()
            rays = max(1, c.total_rays() - c.raysPrimary)
            return {"frame_ms": round(statistics.median(ms), 3),
                    "node_visits_per_ray": round((c.nodeVisitsClosest + c.nodeVisitsShadow) / rays, 3),
                    "tri_tests_per_ray": round((c.triTestsClosest + c.triTestsShadow) / rays, 3),
                    "alpha_tests_per_ray": round((c.alphaTestsClosest + c.alphaTestsShadow) / rays, 4),
                    "hintedNee": int(c.hintedNee), "hintedSplat": int(c.hintedSplat)}

        out = {"shape": name, "triangles": int(d.numTriangles), "sway_vertices": int(sway.sum())}
        trees = {"as_built": frames()}
        poses_dev = [torch.from_numpy(pose(t)).cuda() for t in (3, 7)]
        poses_host = [pose(t) for t in (3, 7)]
        pipe.ctx.prepare(pkg.abi.PREPARE_REFIT)

        def update_times(mems):
            upd = {}
            for mem in mems:
                for keep in (False, True):
                    ms, wall = [], []
                    for r in range(2 + args.reps):
                        p = (poses_dev if mem == "device" else poses_host)[r % 2]
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        t0 = time.perf_counter()
                        e0.record(st)
                        pipe.ctx.update_geometry(p, stream=C.c_void_p(st.cuda_stream), keep_light_maps=keep)
                        e1.record(st)
                        t1 = time.perf_counter()
                        torch.cuda.synchronize()
                        if r >= 2:
                            ms.append(e0.elapsed_time(e1))
                            wall.append((t1 - t0) * 1e3)
                    k = f"{mem}_{'keep_maps' if keep else 'retrace_maps'}"
                    upd[k] = {"device_ms": round(statistics.median(ms), 3)}
                    if mem == "host":
                        upd[k]["call_wall_ms"] = round(statistics.median(wall), 3)
            return upd

        upd = update_times(("device", "host"))
        out["update_ms"] = upd
        for t in range(30):  # the sway, light maps kept (the per-frame animation setting)
            pipe.update_geometry(torch.from_numpy(pose(t + 1)).cuda(), keep_light_maps=True)
        torch.cuda.synchronize()
        trees["after_sway"] = frames()
        info = pipe.ctx.refit_info()
        out["sah_ratio"] = round(info.sahCost / info.sahCostBuilt, 4)
        out["sah"] = {"built": info.sahCostBuilt, "swayed": info.sahCost}
        pfinal = pose(30)
        dm = pkg.abi.SceneDesc()
        C.pointer(dm)[0] = d
        dm.positions = pfinal.ctypes.data_as(C.POINTER(C.c_float))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe.ctx.set_scene(dm)
        torch.cuda.synchronize()
        out["set_scene_s"] = round(time.perf_counter() - t0, 3)
        trees["rebuilt"] = frames()
        out["trees"] = trees
        out["refit_over_set_scene"] = round(upd["device_keep_maps"]["device_ms"] / (out["set_scene_s"] * 1e3), 5)
        if args.pieces:  # the rebuilt tree has seen no update: the regions come from it
            pipe.ctx.prepare(pkg.abi.PREPARE_REFIT)  # (the plan, as for the plain refit: not part of the figure)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipe.ctx.prepare(refit_pieces=True)
            torch.cuda.synchronize()
            bi = pipe.ctx.bvh_info()
            pc = {"prepare_ms": round((time.perf_counter() - t0) * 1e3, 3), "table_bytes": 24 * (int(bi.numNodes) + int(bi.numReferences) + 4)}
            pc["update_ms"] = update_times(("device",))
            for t in range(30):
                pipe.update_geometry(torch.from_numpy(pose(t + 1)).cuda(), keep_light_maps=True)
            torch.cuda.synchronize()
            trees["after_sway_pieces"] = frames()
            info = pipe.ctx.refit_info()
            pc["sah_ratio"] = round(info.sahCost / info.sahCostBuilt, 4)
            pc["refit_over_set_scene"] = round(pc["update_ms"]["device_keep_maps"]["device_ms"] / (out["set_scene_s"] * 1e3), 5)
            out["pieces"] = pc
        print(json.dumps(out), flush=True)
        pipe.close()
        scene.close()
        del poses_dev
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
