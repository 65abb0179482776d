"""Cost of masked frames (bdpt_execute_masked) and a convergence run of adaptive sampling on the bench frame: the
262 k-triangle atrium at 1920x1080, depth 8, GGX.  One JSON line:

  frames        the G-buffer is rendered once; bdpt_execute ("plain") and bdpt_execute_masked at 100 / 50 / 25 / 10 / 0 %
                active (seeded masks of 8 x 8 blocks) run interleaved, --reps times each after --warmup, MIS off and on,
                timed by torch.cuda events around each call on its stream: median, min and max ms per variant
  convergence   FramePipeline(adaptive=<settings>) from a reset until active_pixels() is 0 (or --max-frames): the active
                fraction after every frame, the frames taken and their summed device time (events around each
                render_frame: G-buffer + masked frame + update), and the same for as many plain accumulated frames

  python tools/adaptive_times.py [--reps 15] [--warmup 3] [--max-frames 300] [--settings '{"threshold": 0.05}']
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H, D = 1920, 1080, 8
FRACTIONS = (1.0, 0.5, 0.25, 0.1, 0.0)


def _block_mask(rng, frac, B=8):
    blocks = rng.random(((H + B - 1) // B, (W + B - 1) // B)) < frac
    return np.kron(blocks, np.ones((B, B), bool))[:H, :W].astype(np.uint8)


def _timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def frame_times(torch, pkg, scene, reps, warmup):
    pipe = pkg.FramePipeline(scene, W, H, max_depth=D, mat_index=0)
    st = pipe._stream_ptr()
    pipe.ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, st)
    out = C.c_void_p(pipe.output.data_ptr())
    rng = np.random.default_rng(2024)
    masks = {f: torch.as_tensor(_block_mask(rng, f), device=pipe.dev) for f in FRACTIONS}
    res = {}
    for mis in (False, True):
        p = pipe.bdpt_params(pkg.abi.PARAM_MIS_POWER if mis else 0)
        calls = {"plain": lambda: pipe.ctx.execute(p, pipe.gb, out, st)}
        for f, m in masks.items():
            calls[f"masked_{int(f * 100)}"] = (lambda m=m: pipe.ctx.execute_masked(p, pipe.gb, C.c_void_p(m.data_ptr()), out, st))
        times = {k: [] for k in calls}
        for i in range(warmup + reps):
            for name, fn in calls.items():
                t = _timed(torch, fn)
                if i >= warmup:
                    times[name].append(t)
        key = "mis_power" if mis else "mis_off"
        res[key] = {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
                    for k, v in times.items()}
        res[key]["active_fraction"] = {f"masked_{int(f * 100)}": round(float(m.float().mean()), 4) for f, m in masks.items()}
        plain = res[key]["plain"]["median_ms"]
        res[key]["all_ones_extra_pct"] = round(100.0 * (res[key]["masked_100"]["median_ms"] - plain) / plain, 2)
    pipe.close()
    return res


def convergence(torch, pkg, scene, settings, max_frames):
    pipe = pkg.FramePipeline(scene, W, H, max_depth=D, mat_index=0, adaptive=settings)
    fractions, ms = [], []
    for _ in range(max_frames):
        ms.append(_timed(torch, pipe.render_frame))
        fractions.append(round(pipe.active_pixels() / (W * H), 5))
        if fractions[-1] == 0.0:
            break
    pipe.close()
    n = len(fractions)
    plain = pkg.FramePipeline(scene, W, H, max_depth=D, mat_index=0, accum_limit=max(n, 1))
    pms = [_timed(torch, lambda: plain.render_frame(accumulate=True)) for _ in range(n)]
    plain.close()
    return {"settings": dict(pkg.ADAPTIVE_DEFAULTS, **settings), "frames": n, "converged": fractions[-1] == 0.0,
            "adaptive_ms": round(sum(ms), 1), "plain_accumulated_ms": round(sum(pms), 1),
            "frame_ms_first_last": [round(ms[0], 3), round(ms[-1], 3)], "active_fraction": fractions}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-frames", type=int, default=300)
    ap.add_argument("--settings", default="{}", help="JSON dict of ADAPTIVE_DEFAULTS keys for the convergence run")
    ap.add_argument("--skip-frames", action="store_true", help="only the convergence run")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    scene = pkg.Scene.atrium(1, 262144)
    out = {"scene": "atrium", "width": W, "height": H, "depth": D}
    if not a.skip_frames:
        out["frames"] = frame_times(torch, pkg, scene, a.reps, a.warmup)
    out["convergence"] = convergence(torch, pkg, scene, json.loads(a.settings), a.max_frames)
    print(json.dumps(out))
    scene.close()


if __name__ == "__main__":
    main()
