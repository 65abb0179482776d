"""Cost of denoising P planes with one bdpt_bmfr_execute_planes against P bdpt_bmfr_execute calls on P contexts (one
stream), at 1920x1080 on the 262 k-triangle atrium's G-buffer.  Both forms run the same kernels: the "separate" baseline
is the one-plane instance run P times, so at P = 1 the two forms are one and the same work, and for P >= 2 the ratio shows
what sharing the reprojection and the factorisation among the planes saves.  One BDPT frame with light groups is rendered once; plane k
is that frame's plane k % 4 (three lights + emission) scaled by 1 + k / 8, copied fresh before every timed call.  Both
forms run alternately, --reps times each after --warmup, on frames 1, 2, ... of a still camera (every pixel reprojects),
timed by torch.cuda events around the call(s) on the stream.  The default flags plus regression (preprocess + regression +
postprocess, half frame, rank-dropping QR), and the same with stages left out, so that a stage's time is a difference:

  pre = flags PREPROCESS, fit = (PREPROCESS | REGRESSION) - pre, post = all three - (PREPROCESS | REGRESSION)

One JSON line: per P in --planes, planes_ms and separate_ms (median of the whole call / of the P calls), their min and max,
ratio = planes_ms / separate_ms, separate_spread_pct = (max - min) / median of the baseline's own repeats, and the three
stages of either form.

  python tools/bmfr_planes_times.py [--reps 20] [--warmup 3] [--planes 1,2,4,8,18]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H, D = 1920, 1080, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--planes", default="1,2,4,8,18")
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--height", type=int, default=H)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    A = pkg.abi
    w, h = a.width, a.height
    counts = [int(x) for x in a.planes.split(",")]
    scene = pkg.Scene.atrium(1, 262144)
    pipe = pkg.FramePipeline(scene, w, h, max_depth=D, mat_index=0, light_groups=True)
    pipe.render_frame()
    st = pipe._stream_ptr()
    src = torch.cat([pipe.light_groups, pipe.output[None]])[: 4]
    top = max(counts)
    source = torch.stack([src[k % src.shape[0]] * (1.0 + k / 8.0) for k in range(top)])
    work = torch.empty_like(source)
    vp = pkg.view_proj_of_camera(pipe.cam)
    one = pkg.Context(0)
    one.resize(w, h, 0, 1, 1)  # (a band context: the denoiser takes whole-frame buffers whatever the tile)
    singles = []
    full = A.BMFR_PREPROCESS | A.BMFR_REGRESSION | A.BMFR_POSTPROCESS
    stages = {"pre": A.BMFR_PREPROCESS, "pre_fit": A.BMFR_PREPROCESS | A.BMFR_REGRESSION, "all": full}
    res = {"width": w, "height": h, "reps": a.reps, "warmup": a.warmup, "planes": {}}
    for count in counts:
        while len(singles) < count:
            c = pkg.Context(0)
            c.resize(w, h, 0, 1, 1)
            singles.append(c)
        one.bmfr_planes_prepare(count)
        for c in singles[:count]:
            c.bmfr_reset()
        entry = {}
        for name, flags in stages.items():
            times = {"planes": [], "separate": []}
            for i in range(a.warmup + a.reps):
                bp = A.BmfrParams()
                bp.frameNumber, bp.flags = i + 1, flags
                for j in range(16):
                    bp.prevViewProj[j] = vp[j]
                for form in ("planes", "separate"):
                    work[:count].copy_(source[:count])
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    if form == "planes":
                        one.bmfr_execute_planes(bp, pipe.gb, work[:count], None, st)
                    else:
                        for k in range(count):
                            singles[k].bmfr_execute(bp, pipe.gb, C.c_void_p(work[k].data_ptr()), st)
                    e1.record()
                    torch.cuda.synchronize()
                    if i >= a.warmup:
                        times[form].append(e0.elapsed_time(e1))
            entry[name] = {f: (statistics.median(v), min(v), max(v)) for f, v in times.items()}
        pm, sm = entry["all"]["planes"], entry["all"]["separate"]
        stage = lambda f: {"pre": round(entry["pre"][f][0], 3), "fit": round(entry["pre_fit"][f][0] - entry["pre"][f][0], 3),
                           "post": round(entry["all"][f][0] - entry["pre_fit"][f][0], 3)}
        res["planes"][str(count)] = {
            "planes_ms": round(pm[0], 3), "planes_ms_minmax": [round(pm[1], 3), round(pm[2], 3)],
            "separate_ms": round(sm[0], 3), "separate_ms_minmax": [round(sm[1], 3), round(sm[2], 3)],
            "ratio": round(pm[0] / sm[0], 3), "separate_spread_pct": round(100.0 * (sm[2] - sm[1]) / sm[0], 2),
            "planes_stage_ms": stage("planes"), "separate_stage_ms": stage("separate")}
    print(json.dumps(res))
    for c in singles + [one]:
        c.close()
    pipe.close()
    scene.close()


if __name__ == "__main__":
    main()
