"""bdpt_bmfr_execute_planes (include/bdpt.h "Denoised planes"): P images over one G-buffer through one call, each left with
the bits bdpt_bmfr_execute (bdpt_bmfr_execute_motion) gives it on a context of its own.  Every comparison is bit for bit
(NaN == NaN, as test_bmfr._assert_same): against the CPU oracle, one OracleBmfr per plane, where the oracle can run the case,
and against P separate GPU contexts otherwise."""
import ctypes as C

import numpy as np
import pytest

from test_bmfr import _assert_same, _params, _plane_scene

pytestmark = pytest.mark.gpu

F = np.float32


def make_planes(noisy, count, w_per_plane=False):
    """`count` images from one [H*W, 4] image: channel c of plane k = noisy * s[k][c] + o[k][c].  Plane 0 has a zero blue
    channel, the last plane a red channel shifted below zero for most pixels (the fit's r < 0 clamp runs); no two planes are
    proportional (checked).  w_per_plane: w = 1 + k + (pixel % 3) instead of the input's 1."""
    out = []
    for k in range(count):
        a = noisy.copy()
        for c in range(3):
            a[:, c] = noisy[:, c] * F(0.5 + 0.13 * k + 0.07 * c) + F(0.05 * ((k * 7 + c * 3) % 11))
        if k == 0:
            a[:, 2] = 0.0
        if k == count - 1:
            a[:, 0] -= F(0.9)
        if w_per_plane:
            a[:, 3] = 1.0 + k + (np.arange(a.shape[0]) % 3)
        out.append(a)
    for k in range(count):
        for j in range(k):
            x, y = out[k][:, :3].astype(np.float64).ravel(), out[j][:, :3].astype(np.float64).ravel()
            assert not np.allclose(x * (x @ y) / (x @ x), y, rtol=1e-3, atol=1e-6), (j, k)
    return out


class PlanesRun:
    """A context sized with resize (no scene) fed synthetic G-buffers ([H*W, 4] arrays, as test_bmfr._SyntheticBmfr)."""

    def __init__(self, pkg, W, H):
        import torch
        self.torch, self.pkg, self.W, self.H = torch, pkg, W, H
        self.ctx = pkg.Context(0)
        self.ctx.resize(W, H, 0, H, 1)

    def _features(self, g):
        torch = self.torch
        pos, nrm, alb = g[:3]
        self._keep = (torch.from_numpy(pos).cuda(), torch.from_numpy(nrm.astype(np.float16)).cuda(),
                      torch.from_numpy(alb.astype(np.float16)).cuda())
        gb = self.pkg.abi.GBuffer()
        gb.worldPosition, gb.worldNormal, gb.materialDiffuse = [t.data_ptr() for t in self._keep]
        return gb

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def planes(self, p, g, images, prev=None, as_list=False):
        """one bmfr_execute_planes; returns the images after it"""
        torch = self.torch
        gb = self._features(g)
        shape = (self.H, self.W, 4)
        if as_list:
            t = [torch.from_numpy(a.reshape(shape)).cuda() for a in images]
        else:
            t = torch.from_numpy(np.stack([a.reshape(shape) for a in images])).cuda()
        t_prev = None if prev is None else torch.from_numpy(np.ascontiguousarray(prev).reshape(shape)).cuda()
        self.ctx.bmfr_execute_planes(p, gb, t, t_prev, self._stream())
        torch.cuda.synchronize()
        return [x.cpu().numpy().reshape(-1, 4) for x in t]

    def single(self, p, g, image, prev=None):
        """one bmfr_execute (bmfr_execute_motion with prev) on this context's single-image history"""
        torch = self.torch
        gb = self._features(g)
        t = torch.from_numpy(image).cuda()
        if prev is None:
            self.ctx.bmfr_execute(p, gb, C.c_void_p(t.data_ptr()), self._stream())
        else:
            t_prev = torch.from_numpy(np.ascontiguousarray(prev)).cuda()
            self.ctx.bmfr_execute_motion(p, gb, C.c_void_p(t_prev.data_ptr()), C.c_void_p(t.data_ptr()), self._stream())
        torch.cuda.synchronize()
        return t.cpu().numpy()

    def close(self):
        self.ctx.close()


def _flags(A, full=False, keep_ld=False, stages=None):
    stages = A.BMFR_PREPROCESS | A.BMFR_REGRESSION | A.BMFR_POSTPROCESS if stages is None else stages
    return stages | (A.BMFR_FULL_FRAME if full else 0) | (A.BMFR_KEEP_LD_FEATURES if keep_ld else 0)


def _check_against_oracles(pkg, ob, W, H, flags, count, frames, as_list=False):
    import test_bmfr_cross_check as xc
    run = PlanesRun(pkg, W, H)
    oracles = [ob.OracleBmfr(pkg.abi, W, H) for _ in range(count)]
    for k in range(frames):
        g, vp = xc.sequence_gbuffer(pkg, W, H, k)
        p = _params(pkg, k, flags, vp)
        images = make_planes(g[3], count)
        got = run.planes(p, g, images, as_list=as_list)
        for j, orc in enumerate(oracles):
            ref = images[j].copy()
            orc.execute(p, g[0], g[1], g[2], ref)
            _assert_same(got[j], ref, f"frame {k} plane {j} of {count}")
    for orc in oracles:
        orc.close()
    run.close()


# ---- 1. the synthetic sequence against the oracle
@pytest.mark.parametrize("count", [1, 3, 18])
@pytest.mark.parametrize("W,H", [(7, 5), (33, 31)])
@pytest.mark.parametrize("full", [False, True], ids=["half", "full"])
@pytest.mark.parametrize("keep_ld", [False, True], ids=["ignore_ld", "keep_ld"])
def test_planes_synthetic_sequence_matches_oracle(pkg, ob, W, H, full, keep_ld, count):
    """18 frames (every block offset, the wrap of frame % 16) of the moving-then-still sequence through all three stages;
    1 plane, 3 (not a multiple of the planes a workgroup carries together; passed as a list) and BDPT_BMFR_MAX_PLANES."""
    assert pkg.abi.BMFR_MAX_PLANES == 18
    _check_against_oracles(pkg, ob, W, H, _flags(pkg.abi, full, keep_ld), count, 18, as_list=count == 3)


# ---- 2. several blocks, rank-dropping decisions that differ from block to block
@pytest.mark.parametrize("keep_ld", [False, True], ids=["ignore_ld", "keep_ld"])
def test_planes_133x77_matches_oracle(pkg, ob, keep_ld):
    _check_against_oracles(pkg, ob, 133, 77, _flags(pkg.abi, True, keep_ld), 4, 2)


def _check_against_contexts(pkg, W, H, count, frames, params_of, gbuffer_of, prev_of=None, w_per_plane=False, ob=None):
    """the planes call against `count` contexts running bdpt_bmfr_execute (_motion with prev_of) on one image each; with
    `ob` also against one OracleBmfr per plane, as _check_against_oracles"""
    run = PlanesRun(pkg, W, H)
    refs = [PlanesRun(pkg, W, H) for _ in range(count)]
    oracles = [ob.OracleBmfr(pkg.abi, W, H) for _ in range(count)] if ob is not None else []
    changed = False
    for k in range(frames):
        g, p = gbuffer_of(k), params_of(k)
        prev = None if prev_of is None else prev_of(k)
        images = make_planes(g[3], count, w_per_plane)
        got = run.planes(p, g, images, prev)
        for j, ref in enumerate(refs):
            want = ref.single(p, g, images[j].copy(), prev)
            _assert_same(got[j], want, f"frame {k} plane {j}")
        for j, orc in enumerate(oracles):
            ref = images[j].copy()
            orc.execute(p, g[0], g[1], g[2], ref)
            _assert_same(got[j], ref, f"frame {k} plane {j} against the oracle")
        changed = changed or not np.array_equal(got[0], images[0])
    assert changed, "the call left every frame as it was"
    for r in refs + [run] + oracles:
        r.close()


# ---- 3. stage switches
@pytest.mark.parametrize("off", ["regression", "preprocess", "postprocess"])
def test_planes_stage_switches(pkg, ob, off):
    """33x31, three planes, four frames with one stage off, against three contexts running bdpt_bmfr_execute and against
    three oracles (the contexts run the K = 1 instance of the kernels the planes call runs: the oracle is the independent
    side).  With the preprocess stage off w is the caller's, and differs per plane here."""
    import test_bmfr_cross_check as xc
    A = pkg.abi
    W, H = 33, 31
    stages = (A.BMFR_PREPROCESS | A.BMFR_REGRESSION | A.BMFR_POSTPROCESS) & ~{"regression": A.BMFR_REGRESSION,
                                                                             "preprocess": A.BMFR_PREPROCESS,
                                                                             "postprocess": A.BMFR_POSTPROCESS}[off]
    flags = _flags(A, True, False, stages)
    seq = [xc.sequence_gbuffer(pkg, W, H, k) for k in range(4)]
    _check_against_contexts(pkg, W, H, 3, 4, lambda k: _params(pkg, k, flags, seq[k][1]), lambda k: seq[k][0],
                            w_per_plane=off == "preprocess", ob=ob)


# ---- 4. motion
def _moving_plane(W, H):
    """test_motion's synthetic G-buffer: a plane seen head-on, the view-projection that maps it onto its own pixels, and
    previous positions Q: the upper rows moved three pixels along x, a band moved 0.5 in depth, the rest unmoved."""
    rng = np.random.default_rng(12)
    P, nrm, alb, noisy, _ = _plane_scene(W, H, rng)
    Q = P.copy().reshape(H, W, 4)
    Q[:10, :, 0] -= F(0.06)
    Q[10:14, :, 2] += F(0.5)
    vp = np.zeros((4, 4), F)
    vp[0, 0], vp[1, 1], vp[3, 3] = 1.0 / (0.02 * W / 2), 1.0 / (0.02 * H / 2), 1.0
    return (P, nrm, alb, noisy), Q.reshape(-1, 4), list(vp.reshape(-1))


@pytest.mark.parametrize("full", [False, True], ids=["half", "full"])
def test_planes_motion_equals_bmfr_execute_motion(pkg, full):
    """prevPosition != worldPosition over three frames (the second and third reproject through Q): each plane equals
    bdpt_bmfr_execute_motion on a context of its own."""
    W, H = 40, 24
    g, Q, vp = _moving_plane(W, H)
    flags = _flags(pkg.abi, full)
    rng = np.random.default_rng(5)

    def gbuffer_of(k):
        noisy = g[3].copy()
        noisy[:, :3] *= (1.0 + 0.2 * rng.standard_normal((H * W, 3))).astype(F)
        return g[0], g[1], g[2], noisy

    _check_against_contexts(pkg, W, H, 3, 3, lambda k: _params(pkg, k, flags, vp), gbuffer_of, prev_of=lambda k: Q)


def test_planes_motion_with_unmoved_positions_is_the_plain_call(pkg):
    """prevPosition == worldPosition gives the prevPosition = NULL bits (four frames of the moving sequence, all stages)."""
    import test_bmfr_cross_check as xc
    W, H = 40, 24
    flags = _flags(pkg.abi, True)
    plain, equal = PlanesRun(pkg, W, H), PlanesRun(pkg, W, H)
    for k in range(4):
        g, vp = xc.sequence_gbuffer(pkg, W, H, k)
        p = _params(pkg, k, flags, vp)
        images = make_planes(g[3], 3)
        a = plain.planes(p, g, images)
        b = equal.planes(p, g, images, prev=g[0].copy())
        for j in range(3):
            _assert_same(b[j], a[j], f"frame {k} plane {j}")
    plain.close()
    equal.close()


# ---- 5. history bookkeeping
def test_planes_leave_the_single_image_history_alone(pkg):
    """A bdpt_bmfr_execute sequence with planes calls interleaved between its frames (other images, other frame numbers)
    gives the bits it gives without them."""
    import test_bmfr_cross_check as xc
    W, H = 33, 31
    flags = _flags(pkg.abi, True)
    mixed, alone = PlanesRun(pkg, W, H), PlanesRun(pkg, W, H)
    for k in range(4):
        g, vp = xc.sequence_gbuffer(pkg, W, H, k)
        p = _params(pkg, k, flags, vp)
        a = mixed.single(p, g, g[3].copy())
        g2, vp2 = xc.sequence_gbuffer(pkg, W, H, k + 5, seed=3)
        mixed.planes(_params(pkg, k + 5, flags, vp2), g2, make_planes(g2[3], 3))
        _assert_same(a, alone.single(p, g, g[3].copy()), f"frame {k}")
    mixed.close()
    alone.close()


def _sequence(pkg, W, H, flags, k):
    import test_bmfr_cross_check as xc
    g, vp = xc.sequence_gbuffer(pkg, W, H, k)
    return g, _params(pkg, k, flags, vp)


def test_planes_fewer_planes_use_the_first_slots(pkg):
    """three planes, then two, then three again: planes 0 and 1 equal contexts of their own throughout"""
    W, H = 33, 31
    flags = _flags(pkg.abi, True)
    run, refs = PlanesRun(pkg, W, H), [PlanesRun(pkg, W, H) for _ in range(2)]
    for k, count in enumerate([3, 2, 3]):
        g, p = _sequence(pkg, W, H, flags, k)
        images = make_planes(g[3], 3)[:count]
        got = run.planes(p, g, images)
        for j in range(2):
            _assert_same(got[j], refs[j].single(p, g, images[j].copy()), f"frame {k} plane {j}")
    for r in refs + [run]:
        r.close()


@pytest.mark.parametrize("how", ["grow", "reset", "resize"])
def test_planes_history_is_dropped(pkg, how):
    """Two frames of two planes, then the plane count grows past what bdpt_bmfr_planes_prepare allocated /
    bdpt_bmfr_planes_reset / bdpt_resize: the next call, with frameNumber 2, reprojects zeros, as a fresh context's first
    call with frameNumber 2 does."""
    W, H = 33, 31
    flags = _flags(pkg.abi, True)
    run = PlanesRun(pkg, W, H)
    run.ctx.bmfr_planes_prepare(2)
    for k in range(2):
        g, p = _sequence(pkg, W, H, flags, k)
        run.planes(p, g, make_planes(g[3], 2))
    count = 3 if how == "grow" else 2
    if how == "reset":
        run.ctx.bmfr_planes_reset()
    elif how == "resize":
        run.ctx.resize(W, H, 0, H, 1)
    g, p = _sequence(pkg, W, H, flags, 2)
    images = make_planes(g[3], count)
    got = run.planes(p, g, images)
    for j in range(count):
        fresh = PlanesRun(pkg, W, H)
        _assert_same(got[j], fresh.single(p, g, images[j].copy()), f"{how}: plane {j}")
        fresh.close()
    # and the history was there before: without the drop the same call gives other bits
    kept = PlanesRun(pkg, W, H)
    for k in range(2):
        g0, p0 = _sequence(pkg, W, H, flags, k)
        kept.planes(p0, g0, make_planes(g0[3], 2))
    assert not np.array_equal(kept.planes(p, g, images[:2])[0], got[0])
    kept.close()
    run.close()


# ---- 6. rendered frames through FramePipeline
def test_pipeline_denoises_light_groups(pkg):
    """Atrium stand-in 96x54, depth 3, FramePipeline(light_groups=[0, 1, 0], denoise_groups=...), four frames with a moving
    camera: every entry of light_groups_denoised equals a separate context's bdpt_bmfr_execute of that plane, the last that of
    output; the rendered tensors stay as they are."""
    import torch
    A = pkg.abi
    W, H = 96, 54
    scene = pkg.Scene.atrium(3, 20000)
    with pytest.raises(pkg.BdptError, match="light_groups"):
        pkg.FramePipeline(scene, W, H, max_depth=3, mat_index=1, denoise_groups=7)
    flags = A.BMFR_PREPROCESS | A.BMFR_REGRESSION | A.BMFR_POSTPROCESS
    pipe = pkg.FramePipeline(scene, W, H, max_depth=3, mat_index=1, light_groups=[0, 1, 0], denoise_groups=flags)
    assert tuple(pipe.light_groups.shape) == (3, H, W, 4) and tuple(pipe.light_groups_denoised.shape) == (4, H, W, 4)
    refs = [pkg.Context(0) for _ in range(4)]
    for r in refs:
        r.resize(W, H, 0, H, 1)
    base = scene.camera(W / H)
    for k in range(4):
        cam = scene.camera(W / H)
        for i in range(3):
            cam.posW[i] = base.posW[i] + 0.02 * k * base.cameraU[i]
        pipe.cam = cam
        pipe.ctx.set_camera(cam)
        pipe.render_frame()
        bp = pipe.last_denoise_params
        assert bp.frameNumber == k and bp.flags == flags
        if k > 0:
            assert list(bp.prevViewProj) == prev_vp
        prev_vp = pkg.view_proj_of_camera(cam)
        images = [pipe.light_groups[j] for j in range(3)] + [pipe.output]
        for j, (ctx, image) in enumerate(zip(refs, images)):
            want = image.clone()
            ctx.bmfr_execute(bp, pipe.gb, C.c_void_p(want.data_ptr()), pipe._stream_ptr())
            torch.cuda.synchronize()
            got = pipe.light_groups_denoised[j].cpu().numpy().reshape(-1, 4)
            _assert_same(got, want.cpu().numpy().reshape(-1, 4), f"frame {k} entry {j}")
            assert not np.array_equal(got, image.cpu().numpy().reshape(-1, 4)), f"frame {k} entry {j}: not denoised"
    assert float(pipe.light_groups_denoised[0].abs().sum()) > 0 and float(pipe.light_groups_denoised[1].abs().sum()) > 0
    for r in refs:
        r.close()
    pipe.close()
    scene.close()


# ---- 7. error conventions
def test_planes_error_conventions(pkg):
    """Every refusal of include/bdpt.h "Denoised planes"; after each one the next valid call gives what it gives on a
    context that never saw a refusal: nothing was enqueued, no history slot or ping-pong side moved."""
    import torch
    A, lib = pkg.abi, pkg.load_library()
    INVALID, STATE = -1, -2
    W, H = 33, 31
    flags = _flags(A, True)
    run, clean = PlanesRun(pkg, W, H), PlanesRun(pkg, W, H)
    g0, p0 = _sequence(pkg, W, H, flags, 0)
    gb = run._features(g0)
    feats = run._keep
    buf = torch.zeros(3 * H * W * 4 + 8, dtype=torch.float32, device="cuda")  # room for two planes and shifted ones
    base, plane_bytes = buf.data_ptr(), H * W * 16
    st = run._stream()

    def desc(ptrs, num=None, reserved=0, prev=None):
        d = A.BmfrPlanesDesc()
        arr = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        d.planes = C.cast(arr, C.POINTER(C.c_void_p))
        d.numPlanes = len(ptrs) if num is None else num
        d.reserved, d.prevPosition = reserved, prev
        d._keep = arr
        return d

    good = [base, base + plane_bytes]
    no_size = pkg.Context(0)
    assert lib.bdpt_bmfr_execute_planes(no_size._h, C.byref(p0), C.byref(gb), C.byref(desc(good)), st) == STATE
    assert lib.bdpt_bmfr_planes_prepare(no_size._h, 2) == STATE
    assert lib.bdpt_bmfr_planes_reset(no_size._h) == 0
    no_size.close()
    h = run.ctx._h
    no_normal = A.GBuffer()
    no_normal.worldPosition, no_normal.materialDiffuse = gb.worldPosition, gb.materialDiffuse
    refusals = [
        ("NULL context", lambda: lib.bdpt_bmfr_execute_planes(None, C.byref(p0), C.byref(gb), C.byref(desc(good)), st)),
        ("NULL params", lambda: lib.bdpt_bmfr_execute_planes(h, None, C.byref(gb), C.byref(desc(good)), st)),
        ("NULL features", lambda: lib.bdpt_bmfr_execute_planes(h, C.byref(p0), None, C.byref(desc(good)), st)),
        ("NULL desc", lambda: lib.bdpt_bmfr_execute_planes(h, C.byref(p0), C.byref(gb), None, st)),
        ("missing channel", lambda: lib.bdpt_bmfr_execute_planes(h, C.byref(p0), C.byref(no_normal), C.byref(desc(good)), st)),
        ("no planes", lambda: lib.bdpt_bmfr_execute_planes(h, C.byref(p0), C.byref(gb), C.byref(desc(good, num=0)), st)),
        ("too many planes", lambda: lib.bdpt_bmfr_execute_planes(h, C.byref(p0), C.byref(gb),
                                                                 C.byref(desc(good, num=A.BMFR_MAX_PLANES + 1)), st)),
        ("reserved", lambda: lib.bdpt_bmfr_execute_planes(h, C.byref(p0), C.byref(gb), C.byref(desc(good, reserved=1)), st)),
        ("NULL plane", lambda: lib.bdpt_bmfr_execute_planes(h, C.byref(p0), C.byref(gb), C.byref(desc([base, None])), st)),
        ("misaligned plane", lambda: lib.bdpt_bmfr_execute_planes(h, C.byref(p0), C.byref(gb),
                                                                  C.byref(desc([base, base + plane_bytes + 4])), st)),
        ("misaligned prevPosition", lambda: lib.bdpt_bmfr_execute_planes(h, C.byref(p0), C.byref(gb),
                                                                         C.byref(desc(good, prev=feats[0].data_ptr() + 8)), st)),
        ("the same plane twice", lambda: lib.bdpt_bmfr_execute_planes(h, C.byref(p0), C.byref(gb), C.byref(desc([base, base])), st)),
        ("overlapping planes", lambda: lib.bdpt_bmfr_execute_planes(h, C.byref(p0), C.byref(gb),
                                                                    C.byref(desc([base, base + plane_bytes - 16])), st)),
        ("prepare: no planes", lambda: lib.bdpt_bmfr_planes_prepare(h, 0)),
        ("prepare: too many planes", lambda: lib.bdpt_bmfr_planes_prepare(h, A.BMFR_MAX_PLANES + 1)),
    ]
    assert lib.bdpt_bmfr_planes_prepare(None, 2) == INVALID and lib.bdpt_bmfr_planes_reset(None) == INVALID
    for k, (label, call) in enumerate(refusals):
        buf.fill_(0.25)
        assert call() == INVALID, label
        torch.cuda.synchronize()
        assert bool((buf == 0.25).all()), f"{label}: the refused call wrote the planes"
        g, p = _sequence(pkg, W, H, flags, k)
        images = make_planes(g[3], 2)
        got, want = run.planes(p, g, images), clean.planes(p, g, images)
        for j in range(2):
            _assert_same(got[j], want[j], f"after '{label}': frame {k} plane {j}")
    # the binding refuses before the library is called
    g, p = _sequence(pkg, W, H, flags, 0)
    t = torch.zeros(2, H, W, 4, device="cuda")
    for bad, match in ((t.double(), "float32"), (t[:, :, ::2], "contiguous"), (t.cpu(), "GPU tensor"), (t[:, :, :, :3], "float32"),
                       (torch.zeros(2, H + 1, W, 4, device="cuda"), "whole frames"), ([], "planes"),
                       ([t[0], t[1].double()], "float32"), (torch.zeros(19, H, W, 4, device="cuda"), "planes")):
        with pytest.raises(pkg.BdptError, match=match):
            run.ctx.bmfr_execute_planes(p, gb, bad, None, st)
    with pytest.raises(pkg.BdptError, match="prev_position"):
        run.ctx.bmfr_execute_planes(p, gb, t, torch.zeros(H, W, 3, device="cuda"), st)
    run.close()
    clean.close()
