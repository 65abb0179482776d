"""Costs of area lights (BDPT_PARAM_AREA_LIGHTS): frame time and the gen_nee / init_paths stages with and without the
switch on the Cornell box and the atrium at 1920x1080 depth 8, and the emitter table's build (bdpt_prepare) and refresh
(bdpt_update_geometry's extra kernels) for the atrium and an all-emissive triangle soup.  Prints one JSON line per case.

  python tools/area_light_times.py [--frames N] [--soup-triangles N]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def frame_times(pkg, scene, name, frames):
    import torch
    pipe = pkg.FramePipeline(scene, 1920, 1080, max_depth=8, mat_index=0)
    pipe.ctx.prepare(pkg.abi.PREPARE_AREA_LIGHTS)
    info = pipe.ctx.area_light_info()
    for flags in (0, pkg.abi.PARAM_AREA_LIGHTS):
        for _ in range(3):
            pipe.render_frame(extra_flags=flags)
        torch.cuda.synchronize()
        pipe.ctx.enable_stage_timing(True)
        stages = {}
        t0 = time.perf_counter()
        for _ in range(frames):
            pipe.render_frame(extra_flags=flags)
            torch.cuda.synchronize()
            for k, v in pipe.ctx.stage_times():
                stages[k] = stages.get(k, 0.0) + v
        ms = (time.perf_counter() - t0) * 1e3 / frames
        pipe.ctx.enable_stage_timing(False)
        print(json.dumps({"scene": name, "area_lights": bool(flags), "emitters": info.numEmitters, "frame_ms_wall": round(ms, 3),
                          "gen_nee_ms": round(stages.get("gen_nee", 0.0) / frames, 4),
                          "init_paths_ms": round(stages.get("init_paths", 0.0) / frames, 4),
                          "walk_ms": round(stages.get("walk", 0.0) / frames, 4)}), flush=True)
    pipe.close()


def table_times(pkg, scene, name, reps=20):
    import numpy as np
    import torch
    ctx = pkg.Context(0)
    ctx.set_scene(scene.desc)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctx.prepare(pkg.abi.PREPARE_AREA_LIGHTS)
    build_ms = (time.perf_counter() - t0) * 1e3
    info = ctx.area_light_info()
    d = scene.desc
    p = torch.from_numpy(np.ctypeslib.as_array(d.positions, shape=(int(d.numVertices) * 3,)).copy()).cuda()
    ctx.prepare(pkg.abi.PREPARE_REFIT)
    plain = pkg.Context(0)  # the same update on a context without the table
    plain.set_scene(d)
    plain.prepare(pkg.abi.PREPARE_REFIT)
    res = {}
    for label, c in (("update_with_table", ctx), ("update_without_table", plain)):
        c.update_geometry(p, keep_light_maps=True)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            c.update_geometry(p, keep_light_maps=True, stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
        e1.record()
        torch.cuda.synchronize()
        res[label] = e0.elapsed_time(e1) / reps
    print(json.dumps({"scene": name, "triangles": int(d.numTriangles), "emitters": info.numEmitters, "build_ms_wall": round(build_ms, 3),
                      "update_with_table_ms": round(res["update_with_table"], 4),
                      "update_without_table_ms": round(res["update_without_table"], 4),
                      "refresh_ms": round(res["update_with_table"] - res["update_without_table"], 4)}), flush=True)
    ctx.close()
    plain.close()


class Emissive:
    """a scene whose every material emits a constant (the soup as an all-emissive stress case)"""

    def __init__(self, pkg, scene):
        self.scene = scene
        d = scene.desc
        n = int(d.numMaterials)
        self.mats = (pkg.abi.Material * n)()
        for i in range(n):
            self.mats[i] = d.materials[i]
            self.mats[i].emissive[0] = self.mats[i].emissive[1] = self.mats[i].emissive[2] = 1.0
            self.mats[i].flags = (self.mats[i].flags & ~(7 << 9)) | (1 << 9)
        self.desc = pkg.abi.SceneDesc()
        C.pointer(self.desc)[0] = d
        self.desc.materials = C.cast(self.mats, C.POINTER(pkg.abi.Material))

    def camera(self, aspect):
        return self.scene.camera(aspect)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--soup-triangles", type=int, default=1 << 20)
    a = ap.parse_args()
    pkg = ge.load_package()
    cornell, atrium = pkg.Scene.cornell(), pkg.Scene.atrium(1, 262144)
    frame_times(pkg, cornell, "cornell", a.frames)
    frame_times(pkg, atrium, "atrium", a.frames)
    table_times(pkg, atrium, "atrium")
    soup = pkg.Scene.soup(7, a.soup_triangles, 0.01)
    table_times(pkg, Emissive(pkg, soup), "soup (all emissive)")


if __name__ == "__main__":
    main()
