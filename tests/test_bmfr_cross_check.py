"""The BMFR oracle (oracle/bmfr_oracle.cpp) against a float64 reading of the reference's shaders
(tests/bmfr_reference_numpy.py) on synthetic G-buffers: the regression at every block offset, both QR variants, half
and full frame, frame sizes down to one smaller than a block offset, and frame numbers at which 32-bit arithmetic
wraps; and the temporal pre/post-process over a moving-then-still camera.  The GPU kernels are pinned to the oracle
bit for bit by tests/test_bmfr.py, so these tests pin them to the shaders too."""
import ctypes as C

import numpy as np
import pytest

import bmfr_reference_numpy as ref

SIZES = [(96, 64), (133, 77), (33, 31), (40, 20), (7, 5)]
SCENES = ["plane", "box", "far"]
# |oracle - reading| <= FIT_RTOL[variant] * (0.01 + |reading|) on RGB.  Worst cases measured over every case of
# test_regression_matches_float64_reading and the large frame numbers:
#   KEEP_LD_FEATURES (plain least squares):  1.9e-6 ('far', 96x64), tolerance 5e-5;
#   default (rank-dropping QR):              5.7e-5 ('far', 133x77), tolerance 6e-4 (10x).  Reflections with
#     |u|^2 < 0.001 are skipped there (every kept column whose residual lies between 0.01 and ~0.016 has one), which
#     leaves the factorisation non-orthogonal and amplifies the kernel's fp32 rounding.
# A reading given the next frame's block offset misses by >= 8.5e-2 in every case checked below.
FIT_RTOL = {False: 6e-4, True: 5e-5}
# the temporal stages: colour and spp relative to the reading
TEMPORAL_RTOL = 1e-5
MARGIN = 1e-5  # an element whose decision margin is below this (relative) is not compared


def synthetic_gbuffer(scene, W, H, seed=0, shadow=False):
    """World position (fp32), normal and albedo (half values widened to fp32) and a noisy colour with spp 1, as
    [H*W, 4] arrays.  'plane': a tilted plane spanning less than one world unit per block (the unscaled feature
    branch); 'box': the corner of a box in world units 0-555, three flat walls (the scaled branch, and constant feature
    columns that the rank-dropping QR removes); 'far': a curved sheet around world coordinate 1e4 (squares near 1e8).
    About 3 % of the pixels have an albedo channel below 0.01 (their demodulated colour is 0).  shadow: a hard shadow
    edge crosses the frame, and blocks across it fit below zero next to it."""
    rng = np.random.default_rng([SCENES.index(scene), W, H, seed])
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    u, v = (x + 0.5) / W, (y + 0.5) / H
    pos = np.zeros((H, W, 3))
    nrm = np.zeros((H, W, 3))
    if scene == "plane":
        pos[..., 0] = (x - W / 2) * 0.02
        pos[..., 1] = (H / 2 - y) * 0.02
        pos[..., 2] = -3.0 + 0.1 * pos[..., 0] - 0.05 * pos[..., 1]
        nrm[...] = np.array([-0.1, 0.05, 1.0]) / np.linalg.norm([-0.1, 0.05, 1.0])
    elif scene == "box":
        left, floor = u < 0.3, (v > 0.7) & (u >= 0.3)
        back = ~left & ~floor
        pos[left] = np.stack([np.zeros(left.sum()), 555 * (1 - v[left]), 555 * (1 - u[left] / 0.3)], -1)
        nrm[left] = (1, 0, 0)
        pos[floor] = np.stack([555 * (u[floor] - 0.3) / 0.7, np.zeros(floor.sum()), 555 * (1 - v[floor]) / 0.3], -1)
        nrm[floor] = (0, 1, 0)
        pos[back] = np.stack([555 * (u[back] - 0.3) / 0.7, 555 * (1 - v[back] / 0.7), np.full(back.sum(), 555.0)], -1)
        nrm[back] = (0, 0, -1)
    elif scene == "far":
        a = 2.0 * u - 1.0
        pos[..., 0] = 1.0e4 + 40.0 * a
        pos[..., 1] = 1.2e4 - 30.0 * v
        pos[..., 2] = -0.9e4 + 15.0 * a * a + 5.0 * v
        n = np.stack([-30.0 * a / 40.0, np.full_like(a, -0.1), np.ones_like(a)], -1)
        nrm[...] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    else:
        raise ValueError(scene)
    alb = np.ones((H, W, 4))
    alb[..., :3] = 0.2 + 0.6 * rng.random((H, W, 3))
    dark = rng.random((H, W)) < 0.03
    alb[dark, rng.integers(0, 3, dark.sum())] = 0.004
    # irradiance smooth in the features, radiance = albedo * irradiance, multiplicative noise
    p = (pos - pos.reshape(-1, 3).mean(0)) / (np.ptp(pos.reshape(-1, 3), axis=0) + 1e-9)
    irr = 0.5 + 0.3 * p[..., 0:1] - 0.2 * p[..., 1:2] + 0.1 * p[..., 2:3] ** 2 + 0.1 * nrm[..., 1:2]
    if shadow:
        irr = irr * (u + 0.5 * v > 0.6)[..., None]
    noisy = np.ones((H, W, 4))
    noisy[..., :3] = alb[..., :3] * irr * (1.0 + 0.3 * rng.standard_normal((H, W, 3)))
    f32 = lambda a: np.ascontiguousarray(a, np.float32).reshape(-1, 4)
    half = lambda a: f32(a.astype(np.float16))
    return (f32(np.concatenate([pos, np.ones((H, W, 1))], -1)), half(np.concatenate([nrm, np.zeros((H, W, 1))], -1)),
            half(alb), f32(noisy))


def params(pkg, frame, flags, vp=None):
    p = pkg.abi.BmfrParams()
    p.frameNumber, p.flags = frame, flags
    vp = vp if vp is not None else [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
    for i in range(16):
        p.prevViewProj[i] = vp[i]
    return p


def oracle_fit(pkg, ob, W, H, frame, flags, g):
    """One regression-only execute of a fresh oracle; returns its output."""
    pos, nrm, alb, noisy = g
    out = noisy.copy()
    b = ob.OracleBmfr(pkg.abi, W, H)
    b.execute(params(pkg, frame, flags | ref.REGRESSION), pos, nrm, alb, out)
    b.close()
    return out


def fit_tol(flags):
    return FIT_RTOL[bool(flags & ref.KEEP_LD_FEATURES)]


def fit_error(out, want, margin):
    """(worst |o - r| / (0.01 + |r|) on RGB over the compared pixels, number of w mismatches, pixels skipped)."""
    ok = margin >= MARGIN
    rgb = np.abs(out[ok, :3] - want[ok, :3]) / (0.01 + np.abs(want[ok, :3]))
    w_bad = int(np.sum(out[:, 3] != want[:, 3].astype(np.float32)))
    return (float(rgb.max()) if rgb.size else 0.0), w_bad, int((~ok).sum())


VARIANTS = {"ignore_ld_half": 0, "ignore_ld_full": ref.FULL_FRAME, "keep_ld_half": ref.KEEP_LD_FEATURES,
            "keep_ld_full": ref.KEEP_LD_FEATURES | ref.FULL_FRAME}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("W,H", SIZES)
def test_regression_matches_float64_reading(pkg, ob, W, H, scene, variant):
    """Frames 0-17 (all 16 block offsets and the wrap of frame % 16) of the fit alone: the oracle within FIT_RTOL of
    the float64 least-squares reading on RGB, w exactly; pixels outside the dispatch untouched."""
    flags = VARIANTS[variant]
    g = synthetic_gbuffer(scene, W, H)
    skipped, written = 0, 0
    for frame in range(18):
        out = oracle_fit(pkg, ob, W, H, frame, flags, g)
        want, margin = ref.fit(W, H, frame, flags | ref.REGRESSION, *g)
        err, w_bad, sk = fit_error(out, want, margin)
        assert w_bad == 0, f"frame {frame}: {w_bad} pixels with another w"
        assert err <= fit_tol(flags), f"frame {frame}: worst relative error {err:.3e}"
        untouched = np.isinf(margin)
        assert np.array_equal(out[untouched], g[3][untouched]), f"frame {frame}: a pixel outside the dispatch changed"
        skipped, written = skipped + sk, written + int((~untouched).sum())
    assert skipped <= 0.01 * written, (skipped, written)
    assert written > 0


@pytest.mark.parametrize("variant", ["ignore_ld_full", "keep_ld_half"])
@pytest.mark.parametrize("scene", SCENES)
def test_reading_rejects_the_next_frames_block_offset(pkg, ob, scene, variant):
    """The reading has teeth: given the block offset of frame k+1 it misses the oracle's frame k by far more than
    the tolerance, so the tolerance cannot silently grow to the size of a real mistake."""
    W, H = 96, 64
    flags = VARIANTS[variant]
    g = synthetic_gbuffer(scene, W, H)
    for frame in (0, 7, 15):
        out = oracle_fit(pkg, ob, W, H, frame, flags, g)
        wrong, margin = ref.fit(W, H, frame, flags | ref.REGRESSION, *g, offset_frame=frame + 1)
        ok = np.isfinite(margin)
        rel = np.abs(out[ok, :3] - wrong[ok, :3]) / (0.01 + np.abs(wrong[ok, :3]))
        assert rel.max() >= 1e-2, (frame, rel.max())


@pytest.mark.parametrize("variant", ["ignore_ld_half", "keep_ld_full"])
def test_regression_clamps_negative_fits_at_zero(pkg, ob, variant):
    """Blocks across a hard shadow edge fit below zero next to it: wherever the reading's unclamped fit is clearly
    negative, the oracle writes exactly 0 (regressionCP.hlsl:495-497 clamps before re-modulating by albedo).  The
    tolerance sweep above leaves this scene out: next to a zero crossing (0.01 + |r|) turns the ordinary fp32 error
    of a fit into a large relative one."""
    W, H = 96, 64
    flags = VARIANTS[variant]
    g = synthetic_gbuffer("box", W, H, shadow=True)
    clamped = 0
    for frame in (0, 6, 13):
        out = oracle_fit(pkg, ob, W, H, frame, flags, g)
        raw, margin = ref.fit(W, H, frame, flags | ref.REGRESSION, *g, clamp=False)
        neg = np.isfinite(margin)[:, None] & (raw[:, :3] < -1e-3)
        assert np.all(out[:, :3][neg] == 0.0), (frame, out[:, :3][neg & (out[:, :3] != 0)][:4])
        clamped += int(neg.sum())
    assert clamped > 100, clamped


# frame numbers where the 32-bit arithmetic of the noise hash and of frame % 16 wrap or overflow
LARGE_FRAMES = [161318, 161319, 161320, 161321, 2**31 - 1, 2**31 + 5, 2**32 - 1]


@pytest.mark.parametrize("variant", ["ignore_ld_full", "keep_ld_full"])
def test_regression_at_large_frame_numbers(pkg, ob, variant):
    """mAccumCount counts up without a cap while the camera is still.  frame % 16 is unsigned in the shader and the
    noise-hash index wraps; the oracle once computed both in int (signed overflow from frame 161,319, and a negative
    offset-table index from 2^31)."""
    flags = VARIANTS[variant]
    W, H = 64, 48
    g = synthetic_gbuffer("box", W, H)
    for frame in LARGE_FRAMES:
        out = oracle_fit(pkg, ob, W, H, frame, flags, g)
        want, margin = ref.fit(W, H, frame, flags | ref.REGRESSION, *g)
        err, w_bad, sk = fit_error(out, want, margin)
        assert w_bad == 0 and err <= fit_tol(flags) and sk == 0, (frame, err, w_bad, sk)


# ---- temporal pre/post-process ----

JITTERS = [(0.2, 0.65), (0.8, 0.35), (0.35, 0.2), (0.65, 0.8)]  # sample offsets in the pixel, away from its centre


def sequence_pose(k, moving=8):
    """Camera pose of frame k: a pan and dolly for the first `moving` frames, then still (spp climbs to both caps)."""
    t = min(k, moving - 1)
    return (0.06 * t, 0.02 * t, -3.0 + 0.03 * t), (0.04 * t, 0.0, 0.0), (0.0, 1.0, 0.0)


def sequence_gbuffer(pkg, W, H, k, moving=8, seed=0):
    """Frame k of a synthetic sequence, [H*W, 4] arrays as synthetic_gbuffer, plus prevViewProj (the previous pose,
    identity on frame 0).  A back wall z = 0 at pixel footprints of ~0.07 (the 0.1 position limit falls between
    neighbouring taps) with a box face at z = -0.6 in front of part of it; normals that turn with x faster and faster
    (the normal limit falls between taps somewhere); a patch of points behind the previous camera (w < 0); jittered
    sample positions, so a still camera reprojects pixel 0 to prev_frame_pixel_f = jitter - 0.5 in (-0.5, 0)."""
    aspect = W / H
    cam = sequence_pose(k, moving)
    vp = np.array(pkg.camera_view_proj(*cam, 21.0, 24.0, aspect), np.float64).reshape(4, 4)
    inv = np.linalg.inv(vp)
    jx, jy = JITTERS[k % len(JITTERS)]
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    ndc = np.stack([2 * (x + jx) / W - 1, 1 - 2 * (y + jy) / H], -1)

    def unproject(z):
        q = np.concatenate([ndc, np.full((H, W, 1), z), np.ones((H, W, 1))], -1) @ inv.T
        return q[..., :3] / q[..., 3:]

    o, d = unproject(0.0), unproject(0.5)
    d = d - o

    def hit(zp):
        return o + d * ((zp - o[..., 2]) / d[..., 2])[..., None]

    pos = hit(0.0)
    box = hit(-0.6)
    on_box = (box[..., 0] > 0.2) & (box[..., 0] < 0.8) & (box[..., 1] > -0.6) & (box[..., 1] < 0.3)
    pos[on_box] = box[on_box]
    a = 3.0 * pos[..., 0] * np.abs(pos[..., 0]) + 2.0 * pos[..., 1]
    nrm = np.stack([np.sin(a), 0.3 * np.sin(2 * a), -np.cos(a)], -1)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    # points behind the previous camera: positions the current G-buffer may hold (a moving object, say) that lie
    # behind the last pose; some reproject into [0,1] through the negative w
    prev = sequence_pose(max(k - 1, 0), moving)
    fwd = np.array(prev[1]) - np.array(prev[0])
    fwd /= np.linalg.norm(fwd)
    r0, c0 = max(0, H - 8), min(2, W - 1)
    r1, c1 = max(r0 + 1, H - 2), min(W, c0 + max(1, W // 3))
    py, px = np.mgrid[0:r1 - r0, 0:c1 - c0].astype(np.float64)
    behind = np.array(prev[0]) - 1.5 * fwd + np.stack([0.15 * (px - W / 6), 0.2 * (py - 3), 0.05 * px], -1)
    pos[r0:r1, c0:c1] = behind
    rng = np.random.default_rng([W, H, k, seed])
    noisy = np.ones((H, W, 4))
    noisy[..., :3] = 0.1 + rng.random((H, W, 3))
    alb = np.ones((H, W, 4))
    alb[..., :3] = 0.5
    f32 = lambda a: np.ascontiguousarray(a, np.float32).reshape(-1, 4)
    half = lambda a: f32(a.astype(np.float16))
    g = (f32(np.concatenate([pos, np.ones((H, W, 1))], -1)), half(np.concatenate([nrm, np.zeros((H, W, 1))], -1)),
         half(alb), f32(noisy))
    prev_vp = None if k == 0 else pkg.camera_view_proj(*prev, 21.0, 24.0, aspect)
    return g, prev_vp


def temporal_close(o, r):
    return np.abs(o - r) <= TEMPORAL_RTOL * np.abs(r) + 1e-7


@pytest.mark.parametrize("full", [True, False], ids=["full", "half"])
def test_pre_and_postprocess_sequence_match_float64_reading(pkg, ob, full):
    """22 frames of preprocess + postprocess, the camera moving for 8 and then still: the oracle's preprocessed colour
    and spp and its accumulated colour within 1e-5 relative of the reading, which carries its own history; its
    accept bools exactly.  An element is left out when one of its decisions has a margin below 1e-5, and fewer than
    1 % are; the reading's history takes the oracle's values there, so that a skip does not spread.  Where only the
    RG16Float store of prev_frame_pixel_f lies near a rounding midpoint (midpoints are 2^-10 relative apart, so that
    is ~4 % of moving pixels), the oracle's value must be one of the two candidates and the reading continues with it.
    The sequence must reach both blend caps and place pixels just outside [0,1], on prev_frame_pixel_f in (-0.5, 0),
    behind the previous camera, and on both sides of both limits."""
    W, H, frames = 64, 48, 22
    flags = ref.PREPROCESS | ref.POSTPROCESS | (ref.FULL_FRAME if full else 0)
    b = ob.OracleBmfr(pkg.abi, W, H)
    S = ref.State(W, H)
    n = W * H
    proc = np.ones(n, bool) if full else ~((np.arange(n) % W + 0.5) / W > 0.5)
    skipped = compared = adopted = 0
    seen = dict(just_outside=0, neg_pf=0, behind_inside=0, pd_in=0, pd_out=0, nd_in=0, nd_out=0)
    max_pre_spp = max_post_spp = 0.0
    for k in range(frames):
        g, vp = sequence_gbuffer(pkg, W, H, k)
        out = g[3].copy()
        b.execute(params(pkg, k, flags, vp), g[0], g[1], g[2], out)
        o_noisy, o_accept, o_pixel = b.state()
        frame_state = {}

        def amend(noisy):
            # runs after the reading's preprocess: compare it, then take the oracle's values where it had no margin
            r_pre, m_pre, _ = S.last_pre
            bad = proc & (m_pre < MARGIN)
            ok = proc & ~bad
            assert np.array_equal(o_accept[ok], S.accept[ok]), f"frame {k}: accept bools differ"
            close = temporal_close(o_noisy[ok], r_pre[ok])
            assert close.all(), f"frame {k}: preprocessed colour / spp differ at {(~close).any(1).sum()} pixels"
            if k > 0:
                amb = ok & (S.diag["half_margin"] < MARGIN)
                h = S.prev_pixel[amb].astype(np.float16)
                step = np.maximum(np.nextafter(h, np.float16(np.inf)) - h, h - np.nextafter(h, np.float16(-np.inf)))
                d_pf = np.abs(o_pixel[amb] - S.prev_pixel[amb])
                # one float16 step, or the margin window where steps are finer than that (near 0)
                lim = np.maximum(step.astype(np.float64), MARGIN * np.maximum(1.0, np.abs(S.prev_pixel[amb])))
                assert np.all(d_pf <= lim), (k, d_pf[d_pf > lim])
                S.prev_pixel[amb] = o_pixel[amb]
                frame_state["adopted"] = int(amb.sum())
            S.accept[bad], S.prev_pixel[bad], S.prev_noisy[bad] = o_accept[bad], o_pixel[bad], o_noisy[bad]
            noisy = noisy.copy()
            noisy[bad] = o_noisy[bad]
            frame_state["pre_bad"] = bad
            return noisy

        r_out, st = ref.execute(S, k, flags, vp, *g, amend=amend)
        _, m_post, _ = st["post"]
        post_bad = m_post < MARGIN
        okp = ~post_bad
        close = temporal_close(out[okp], r_out[okp])
        assert close.all(), f"frame {k}: accumulated colour differs at {(~close).any(1).sum()} pixels"
        S.prev_filtered[post_bad] = out[post_bad]
        skipped += int((proc & (frame_state["pre_bad"] | post_bad)).sum())
        compared += int(proc.sum())
        adopted += frame_state.get("adopted", 0)
        if k > 0:
            d = S.diag
            u, v = d["u"], d["v"]
            seen["just_outside"] += int(np.sum(((u > 1) & (u < 1 + 2.0 / W)) | ((u < 0) & (u > -2.0 / W)) |
                                               ((v > 1) & (v < 1 + 2.0 / H)) | ((v < 0) & (v > -2.0 / H))))
            pf = d["pf"]
            seen["neg_pf"] += int(np.sum(d["inside"] & ((pf > -0.5) & (pf < 0)).any(1) & (S.accept > 0)))
            seen["behind_inside"] += int(np.sum(d["inside"] & (d["w"] < 0)))
            pd, nd = d["pd"], d["nd"]
            seen["pd_in"] += int(np.sum((pd < 0.01) & (pd > 0.008)))
            seen["pd_out"] += int(np.sum((pd >= 0.01) & (pd < 0.012)))
            seen["nd_in"] += int(np.sum((nd < 1.0) & (nd > 0.8)))
            seen["nd_out"] += int(np.sum((nd >= 1.0) & (nd < 1.2)))
            r_pre = S.last_pre[0]
            max_pre_spp = max(max_pre_spp, float(r_pre[proc, 3].max()))
            max_post_spp = max(max_post_spp, float(np.where(S.accept[proc] > 0, r_pre[proc, 3], 0).max()))
    b.close()
    assert skipped < 0.01 * compared, (skipped, compared)
    assert adopted < 0.05 * compared, (adopted, compared)
    assert all(v > 0 for v in seen.values()), seen
    assert max_pre_spp >= 5 and max_post_spp >= 10, (max_pre_spp, max_post_spp)
