"""Costs of morph targets (bdpt_set_morph / bdpt_update_morphed) on the BASELINE shapes configs[2] (atrium 262 k) and
configs[4] (courtyard 10 M).  One JSON line per shape, every device time the median of device events after warm-up, all in
one job.  The morph: --targets targets (64) over about --region (10 %) of the vertices, each target on a random
--cover (1/8) of that region; the skin: --bones bones (32), as tools/skin_times.py rigs it.

  kernel_ms        the fused morph + skin kernel alone (bdpt_test_morph_kernel) with 0, 4 and 32 non-zero weights (the
                   path an update takes; with 0 also both palette paths, forced), and the skinning kernel alone
                   (bdpt_test_skin_kernel, the path bdpt_update_skinned takes, and its global-memory gather) on the same
                   rig: the yardstick.  zero_weight_over_skin: their ratio (the morph kernel reads 8 B of `start` per vertex
                   and 4 B of target id per entry on top of the skin kernel's 96 B per vertex)
  update_ms        bdpt_update_morphed (32 non-zero weights) and bdpt_update_skinned with device inputs, light maps kept
  host_route       what bdpt_update_morphed replaces: bdpt_host_morph (morph_wall_ms, the library's threads) and
                   bdpt_update_geometry from host memory (device_ms of the call, call_wall_ms of the finiteness check and
                   the pinned copy), and total_wall_ms from the weights to the device having finished

  python tools/morph_times.py [--configs 2,4 | atrium:N,courtyard:N] [--reps 10]
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


def make_targets(seed, nv, num_targets, region, cover):
    """`num_targets` targets, each on a random `cover` of the first `region` of a random vertex order"""
    rng = np.random.default_rng(seed)
    reg = rng.permutation(nv)[:max(1, int(nv * region))]
    k = max(1, int(reg.size * cover))
    lists = [np.sort(rng.choice(reg, size=k, replace=False)) for _ in range(num_targets)]
    ts = np.zeros(num_targets + 1, np.uint32)
    ts[1:] = np.cumsum([v.size for v in lists])
    vertex = np.concatenate(lists).astype(np.uint32)
    delta = lambda s: (rng.standard_normal((vertex.size, 3), dtype=np.float32) * np.float32(s))
    return ts, vertex, delta, reg.size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,4")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--bones", type=int, default=32)
    ap.add_argument("--targets", type=int, default=64)
    ap.add_argument("--region", type=float, default=0.1)
    ap.add_argument("--cover", type=float, default=0.125)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    import morph_numpy as mn
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
        nb, T = args.bones, args.targets
        ctx = pkg.Context(0)
        ctx.set_scene(d)
        r = sn.scene_rig(d, 5, nb, static_share=0.25)
        poses = [sn.make_pose(s, nb, r["pivot"], r["extent"], angle=0.01, shift=0.002) for s in (1, 2)]
        ts, vertex, delta, region = make_targets(7, nv, T, args.region, args.cover)
        tg = dict(ts=ts, vertex=vertex, dP=delta(0.002 * r["extent"]), dN=delta(0.05), dB=delta(0.05) if r["B"] is not None else None,
                  num_vertices=nv, num_targets=T)
        ctx.set_skin(r["P"], r["W"], r["I"], nb, r["N"], r["B"])
        mn.set_morph(ctx, tg)
        out = {"shape": name, "triangles": int(d.numTriangles), "vertices": nv, "bones": nb, "targets": T, "morphed_vertices": int(region),
               "entries": int(vertex.size), "kernel_ms": {}}

        def weights(nonzero, seed=0):
            w = np.zeros(T, np.float32)
            w[np.random.default_rng(seed).permutation(T)[:nonzero]] = np.float32(0.5)
            return w

        ctx.update_skinned(poses[0][0], poses[0][1], stream=sp, keep_light_maps=True)  # (stages the device palette)
        k = {"skin": round(timed(lambda _: ctx.test_skin_kernel(0, sp)), 4)}
        for nz in (0, 4, 32):
            ctx.update_morphed(weights(nz), poses[0][0], poses[0][1], stream=sp, keep_light_maps=True)  # (stages weights and palettes)
            k[f"morph_{nz}"] = round(timed(lambda _: ctx.test_morph_kernel(0, sp)), 4)
            if nz == 0:  # the two palette paths, forced
                k["morph_0_global"] = round(timed(lambda _: ctx.test_morph_kernel(1, sp)), 4)
                k["morph_0_lds"] = round(timed(lambda _: ctx.test_morph_kernel(2, sp)), 4)
        k["skin_global"] = round(timed(lambda _: ctx.test_skin_kernel(1, sp)), 4)
        k["zero_weight_over_skin"] = round(k["morph_0"] / k["skin"], 3)
        out["kernel_ms"] = k
        dev = [(torch.from_numpy(b).cuda(), torch.from_numpy(t).cuda()) for b, t in poses]
        wdev = [torch.from_numpy(weights(32, s)).cuda() for s in (0, 1)]
        out["update_ms"] = {
            "update_morphed": round(timed(lambda i: ctx.update_morphed(wdev[i % 2], *dev[i % 2], stream=sp, keep_light_maps=True)), 3),
            "update_skinned": round(timed(lambda i: ctx.update_skinned(*dev[i % 2], stream=sp, keep_light_maps=True)), 3)}
        morph_wall = []

        def host_way(i):
            t0 = time.perf_counter()
            rc, p, n, b = mn.host_morph(lib, pkg.abi, tg, weights(32, i % 2), r["P"], r["N"], r["B"], rig=r, bones=poses[i % 2][0],
                                        normal_bones=poses[i % 2][1])
            morph_wall.append((time.perf_counter() - t0) * 1e3)
            ctx.update_geometry(p, n, b, stream=sp, keep_light_maps=True)

        dms, call, total = timed(host_way, wall=True)
        mw = statistics.median(morph_wall[2:])
        out["host_route"] = {"device_ms": round(dms, 3), "morph_wall_ms": round(mw, 3), "call_wall_ms": round(call - mw, 3),
                             "total_wall_ms": round(total, 3)}
        print(json.dumps(out), flush=True)
        ctx.close()
        scene.close()
        del dev, wdev
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
