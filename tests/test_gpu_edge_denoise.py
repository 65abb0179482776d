"""The BMFR kernels (csrc/bmfr.hip behind bdpt_bmfr_execute, _motion and _planes) on the edge-case families of
tests/edge_denoise.py: against the CPU oracle on every float word (two NaNs count as equal: the header promises a NaN, not
which one), the history blob included; every plane of a planes call against a single-image run of its own; the motion
call against the oracle's prevPosition entry point; and against the float64 reading directly.  The oracle itself is pinned
to the reading by tests/test_edge_denoise_cpu.py.  Frames of at most 65x33, four per sequence."""
import ctypes as C

import numpy as np
import pytest

import bmfr_reference_numpy as ref
import edge_denoise as ed
from edge_images import same_bits
from test_gpu_bmfr_planes import PlanesRun

pytestmark = pytest.mark.gpu

F = np.float32


class EdgeRun:
    """One context and one oracle of a frame size, reset between sequences; G-buffers go in as test_bmfr._SyntheticBmfr
    sends them (worldPosition fp32, worldNormal and materialDiffuse as fp16 bit patterns)."""

    def __init__(self, pkg, ob, W, H):
        import torch
        self.torch, self.pkg, self.W, self.H = torch, pkg, W, H
        self.lib = pkg.load_library()
        self.ctx = pkg.Context(0)
        self.ctx.resize(W, H, 0, H, 1)
        self.orc = ob.OracleBmfr(pkg.abi, W, H)

    def reset(self):
        self.ctx.bmfr_reset()
        self.orc.reset()

    def frame(self, p, f):
        """one call on both; returns (gpu image, oracle image)"""
        torch = self.torch
        with np.errstate(invalid="ignore"):  # (narrowing a signalling NaN)
            t = [torch.from_numpy(f["pos"]).cuda(), torch.from_numpy(f["nrm"].astype(np.float16)).cuda(),
                 torch.from_numpy(f["alb"].astype(np.float16)).cuda(), torch.from_numpy(f["noisy"]).cuda()]
        gb = self.pkg.abi.GBuffer()
        gb.worldPosition, gb.worldNormal, gb.materialDiffuse = [x.data_ptr() for x in t[:3]]
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if f["prev_pos"] is None:
            self.ctx.bmfr_execute(p, gb, C.c_void_p(t[3].data_ptr()), stream)
        else:
            t_prev = torch.from_numpy(f["prev_pos"]).cuda()
            self.ctx.bmfr_execute_motion(p, gb, C.c_void_p(t_prev.data_ptr()), C.c_void_p(t[3].data_ptr()), stream)
        torch.cuda.synchronize()
        want = f["noisy"].copy()
        self.orc.execute(p, f["pos"], f["nrm"], f["alb"], want, f["prev_pos"])
        return t[3].cpu().numpy(), want

    def history(self):
        """the blob of bdpt_bmfr_save_history: position, normal, noisy and filtered history as [4, n, 4] float32"""
        n = C.c_uint64()
        assert self.lib.bdpt_bmfr_history_bytes(self.ctx._h, C.byref(n)) == 0 and n.value == self.W * self.H * 64
        blob = np.zeros(n.value // 4, F)
        assert self.lib.bdpt_bmfr_save_history(self.ctx._h, blob.ctypes.data_as(C.c_void_p), n.value) == 0
        return blob.reshape(4, self.W * self.H, 4)

    def close(self):
        self.orc.close()
        self.ctx.close()


def _differ(a, b):
    bad = ~((ed.F(a).view(np.uint32) == ed.F(b).view(np.uint32)) | (np.isnan(a) & np.isnan(b)))
    return f"{int(bad.any(axis=-1).sum())} texels differ, the first at {np.argwhere(bad)[:3].tolist()}"


@pytest.mark.parametrize("W,H", ed.SIZES)
@pytest.mark.parametrize("family", list(ed.FAMILIES))
def test_execute_matches_oracle(pkg, ob, family, W, H):
    """bdpt_bmfr_execute (bdpt_bmfr_execute_motion where the family has a prevPosition channel) over every run and flag set
    of the family: the image after every frame equals the oracle's word for word, and so do the histories the next frame
    reads (the blob's noisy history against oracle_bmfr_state, its position and normal against the inputs, its filtered
    history against the image).  The accept bools and prev_frame_pixel_f are not in the blob: postprocess reads them back
    on the same frame, so the image pins them."""
    run = EdgeRun(pkg, ob, W, H)
    frames_run = 0
    for name, frames in ed.sequences(family, W, H).items():
        for label, flags in ed.flag_sets_of(family, name):
            run.reset()
            for k, f in enumerate(frames):
                fl = flags[k] if isinstance(flags, list) else flags
                got, want = run.frame(ed.params(pkg, k, fl, f["vp"]), f)
                where = f"{family}/{name} {W}x{H} {label} frame {k}"
                assert same_bits(got, want), f"{where}: {_differ(got, want)}"
                hist = run.history()
                noisy = run.orc.state()[0]
                assert same_bits(hist[2], noisy), f"{where}: noisy history: {_differ(hist[2], noisy)}"
                with np.errstate(invalid="ignore"):
                    nrm = f["nrm"].astype(np.float16).astype(F)
                assert same_bits(hist[0], f["pos"]) and same_bits(hist[1], nrm), f"{where}: position / normal history"
                if fl & ref.POSTPROCESS:
                    assert same_bits(hist[3], got), f"{where}: filtered history"
                frames_run += 1
    run.close()
    assert frames_run >= ed.FRAMES * 4


def _plane_images(noisy, count, k):
    """`count` images over one G-buffer, each from another colour family: the ordinary image; special colours; the
    ill-conditioned ones with the spp pole and the 1e9 beside ordinary taps; every special texel a NaN; an image of NaNs
    only.  The special values sit where edge_denoise.deal puts them."""
    H, W = noisy.shape[:2]
    sets = [None,
            [v for v in ed.COLOUR_VARIANTS if not callable(v)],
            ed.COLOUR_ILL_VARIANTS + [(0.3, 0.3, 0.3, -1.0), (0.3, 0.3, 0.3, F(1e9))],
            [(ed.NAN, ed.NAN, ed.NAN, ed.NAN)],
            "all"]
    out = []
    for variants in sets[:count]:
        a = noisy.copy()
        if variants == "all":
            a[...] = ed.NAN
        elif variants is not None:
            v = ed.deal(W, H, k, len(variants))
            for i, val in enumerate(variants):
                a[v == i] = val
        out.append(np.ascontiguousarray(a.reshape(-1, 4)))
    return out


PLANE_FLAGS = {"all/full/ignore_ld": ed.STAGES["all"] | ref.FULL_FRAME,
               "all/half/keep_ld": ed.STAGES["all"] | ref.KEEP_LD_FEATURES,
               "switch_half": [ed.STAGES["all"] | f for f in (0, ref.FULL_FRAME, 0, ref.FULL_FRAME)]}


@pytest.mark.parametrize("count", [1, 2, 3, 5])
@pytest.mark.parametrize("W,H", [(33, 31), (65, 33)])
def test_planes_equal_their_single_image_runs(pkg, W, H, count):
    """bdpt_bmfr_execute_planes with 1, 2, 3 and 5 planes (the fit's instances K = 1, 2, 4, and 4 followed by a partial
    round), each plane from another colour family over ordinary geometry and over background texels seen from the origin:
    every plane equals bdpt_bmfr_execute of that image on a context of its own, word for word.  Over the ordinary geometry
    the first plane, which holds no special value, stays finite: nothing of the NaN planes beside it reaches it."""
    for geometry in ("ordinary", "eye_at_origin"):
        for label, flags in PLANE_FLAGS.items():
            run, singles = PlanesRun(pkg, W, H), [PlanesRun(pkg, W, H) for _ in range(count)]
            for k in range(ed.FRAMES):
                if geometry == "ordinary":
                    f = ed.finish([ed.ordinary(W, H, k)])[0]
                else:
                    f = ed.sequences("background", W, H)[geometry][k]
                fl = flags[k] if isinstance(flags, list) else flags
                p = ed.params(pkg, k, fl, f["vp"])
                g = (f["pos"], f["nrm"], f["alb"])
                images = _plane_images(f["noisy"].reshape(H, W, 4), count, k)
                got = run.planes(p, g, images)
                for j, single in enumerate(singles):
                    want = single.single(p, g, images[j].copy())
                    assert same_bits(got[j], want), f"{geometry} {label} frame {k} plane {j} of {count}: {_differ(got[j], want)}"
                if geometry == "ordinary":
                    assert np.isfinite(got[0]).all(), f"{label} frame {k}: a NaN reached the ordinary plane"
                    if count > 3:
                        assert np.isnan(got[3]).any()
            for r in singles + [run]:
                r.close()


@pytest.mark.parametrize("W,H", ed.SIZES)
def test_motion_with_unmoved_positions_is_the_plain_call(pkg, ob, W, H):
    """prev_pos == pos bit for bit: bdpt_bmfr_execute_motion gives bdpt_bmfr_execute's words (include/bdpt.h)"""
    frames = ed.sequences("motion", W, H)["unmoved"]
    moved, plain = EdgeRun(pkg, ob, W, H), EdgeRun(pkg, ob, W, H)
    for label, flags in ed.flag_sets():
        if not label.startswith(("all/", "temporal/full", "switch_half")):
            continue
        moved.reset()
        plain.reset()
        for k, f in enumerate(frames):
            fl = flags[k] if isinstance(flags, list) else flags
            p = ed.params(pkg, k, fl, f["vp"])
            a, _ = moved.frame(p, f)
            b, _ = plain.frame(p, dict(f, prev_pos=None))
            assert same_bits(a, b), f"{label} frame {k}: {_differ(a, b)}"
    moved.close()
    plain.close()


@pytest.mark.parametrize("family", list(ed.WELL))
def test_gpu_matches_float64_reading(pkg, ob, family):
    """33x31, the well-conditioned families, all three stages and the two temporal ones: the kernels against the reading
    directly, within the tolerances and with the value classes of test_edge_denoise_cpu.py, so that they stay pinned to the
    shaders even if the oracle changes.  (The accept bools and prev_frame_pixel_f a frame leaves are the oracle's, whose
    image the kernels' has just been found equal to.)"""
    W, H = 33, 31
    run = EdgeRun(pkg, ob, W, H)
    tally = ed.Tally()

    def execute(k, p, f):
        got, want = run.frame(p, f)
        assert same_bits(got, want)
        _, accept, pixel = run.orc.state()
        return got, (run.history()[2].copy(), accept, pixel)

    for name, frames in ed.sequences(family, W, H).items():
        for label, flags in ed.flag_sets_of(family, name):
            if label.startswith(("all/", "temporal/full", "fit/full")):
                run.reset()
                ed.run_sequence(tally, f"{family}/{name} {label}", pkg, W, H, flags, frames, execute)
    run.close()
    assert not tally.bad, tally.bad[:8]
    assert tally.classes > 0
    assert tally.fit[False] <= ed.FIT_RTOL[False] and tally.fit[True] <= ed.FIT_RTOL[True] and tally.temporal <= ed.TEMPORAL_RTOL, \
        (tally.fit, tally.temporal)
