"""Costs of skinned animation (bdpt_set_skin / bdpt_update_skinned) on the BASELINE shapes configs[2] (atrium 262 k) and
configs[4] (courtyard 10 M).  One JSON line per shape, every device time the median of device events after warm-up:

  kernel_ms        the skinning kernel alone (bdpt_test_skin_kernel), per palette size: the path bdpt_update_skinned takes
                   ("auto"), the global-memory gather, and the LDS-staged palette where the palette is small enough for it;
                   gbytes_per_s: the bytes the kernel moves (60 B read + 36 B written per vertex with all three streams,
                   plus the palette once) over the "auto" time, and its share of the 6.29 TB/s a float4 copy reaches
  update_skinned   bdpt_update_skinned with device bones: light maps kept / re-traced
  update_geometry  the same animation without skinning on the device:
                     device   bdpt_update_geometry with device pointers (the refit tail alone)
                     host     bdpt_update_geometry with host pointers: device_ms of the call, call_wall_ms of the call
                              (finiteness check + pinned copy), skin_wall_ms of skinning the three streams on the host
                              (bdpt_host_skin, the library's threads), and total_wall_ms from the bones to the device
                              having finished

  python tools/skin_times.py [--configs 2,4 | atrium:N,courtyard:N] [--reps 10] [--bones 32,64,256]
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
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

HBM_COPY_TBS = 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,4")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--bones", default="32,64,256")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    import skin_numpy as sn
    pkg = ge.load_package()
    lib = pkg.load_library()
    shapes = {"2": ("atrium 262k", lambda: pkg.Scene.atrium(1, 262144)),
              "4": ("courtyard 10M", lambda: pkg.Scene.courtyard(1, 10000000))}
    st = torch.cuda.current_stream()
    sp = C.c_void_p(st.cuda_stream)

    def timed(fn, wall=False):
        ms, ws = [], []
        for r in range(2 + args.reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(st)
            fn(r)
            e1.record(st)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if r >= 2:
                ms.append(e0.elapsed_time(e1))
                ws.append(((t1 - t0) * 1e3, (t2 - t0) * 1e3))
        if wall:
            return statistics.median(ms), statistics.median(w[0] for w in ws), statistics.median(w[1] for w in ws)
        return statistics.median(ms)

    for key in args.configs.split(","):
        if ":" in key:  # atrium:N / courtyard:N: the same scene at another triangle count
            kind, tris = key.split(":")
            name, make = f"{kind} {tris}", (lambda k=kind, t=int(tris): getattr(pkg.Scene, k)(1, t))
        else:
            name, make = shapes[key]
        scene = make()
        d = scene.desc
        nv = int(d.numVertices)
        ctx = pkg.Context(0)
        ctx.set_scene(d)
        out = {"shape": name, "triangles": int(d.numTriangles), "vertices": nv, "kernel_ms": {}}
        streams = 3 if d.bitangents else 2
        for nb in [int(x) for x in args.bones.split(",")]:
            r = sn.scene_rig(d, 5, nb, static_share=0.25)
            poses = [sn.make_pose(s, nb, r["pivot"], r["extent"], angle=0.01, shift=0.002) for s in (1, 2)]
            ctx.set_skin(r["P"], r["W"], r["I"], nb, r["N"], r["B"])
            ctx.update_skinned(poses[0][0], poses[0][1], stream=sp, keep_light_maps=True)  # (stages the device palette)
            k = {}
            for label, path in (("auto", 0), ("global", 1), ("lds", 2)):
                if path == 2 and nb > pkg.abi.SKIN_LDS_BONES:
                    continue
                k[label] = round(timed(lambda _: ctx.test_skin_kernel(path, sp)), 4)
            nbytes = nv * (24 + 24 * streams) + nb * 64 * (2 if r["N"] is not None else 1)
            k["gbytes_per_s"] = round(nbytes / (k["auto"] * 1e-3) / 1e9, 1)
            k["share_of_hbm_copy_rate"] = round(k["gbytes_per_s"] / (HBM_COPY_TBS * 1e3), 3)
            out["kernel_ms"][str(nb)] = k
        # the animation, with the last palette size
        dev = [(torch.from_numpy(b).cuda(), torch.from_numpy(t).cuda()) for b, t in poses]
        out["bones"] = nb
        out["update_skinned"] = {
            "device_keep_maps_ms": round(timed(lambda i: ctx.update_skinned(*dev[i % 2], stream=sp, keep_light_maps=True)), 3),
            "device_retrace_maps_ms": round(timed(lambda i: ctx.update_skinned(*dev[i % 2], stream=sp)), 3)}
        skinned = [sn.host_skin(lib, pkg.abi, r["P"], r["W"], r["I"], b, t, r["N"], r["B"])[1:] for b, t in poses]
        sk_dev = [tuple(None if a is None else torch.from_numpy(a).cuda() for a in s) for s in skinned]
        geo = {"device_keep_maps_ms": round(timed(lambda i: ctx.update_geometry(*sk_dev[i % 2], stream=sp, keep_light_maps=True)), 3)}
        skin_wall = []

        def host_way(i):
            t0 = time.perf_counter()
            rc, p, n, b = sn.host_skin(lib, pkg.abi, r["P"], r["W"], r["I"], poses[i % 2][0], poses[i % 2][1], r["N"], r["B"])
            skin_wall.append((time.perf_counter() - t0) * 1e3)
            ctx.update_geometry(p, n, b, stream=sp, keep_light_maps=True)

        dms, call, total = timed(host_way, wall=True)
        sw = statistics.median(skin_wall[2:])
        geo["host_keep_maps"] = {"device_ms": round(dms, 3), "skin_wall_ms": round(sw, 3), "call_wall_ms": round(call - sw, 3),
                                 "total_wall_ms": round(total, 3)}
        out["update_geometry"] = geo
        print(json.dumps(out), flush=True)
        ctx.close()
        scene.close()
        del dev, sk_dev
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
