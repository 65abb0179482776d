"""Edge-case G-buffers and histories for the BMFR denoiser (tests/test_edge_denoise_cpu.py, tests/test_gpu_edge_denoise.py):
seeded sequences of FRAMES frames of (pos, nrm, alb, noisy[, prev_pos], view_proj), and the frame-by-frame comparison of an
implementation (the oracle, or the kernels) with the float64 reading of tests/bmfr_reference_numpy.py.  Plain numpy, no
product code.

Every family puts its special texels beside ordinary ones: single pixels along the bottom row and the right column, one
row, and one block of up to 32x32 texels in the top left corner, so that a failure shows whether the damage stays where
the shader confines it.  The special values are dealt over those places and move from frame to frame.

What the shaders do with such texels (line numbers of the reference's Data/ directory):
  preprocess.ps.hlsl:64-73    a NaN prev_frame_uv passes the "outside" test (every comparison is false); int2() of it
                              (:80) is D3D's ftoi, 0, so the four taps around pixel (0,0) are tested (:101-140)
  preprocess.ps.hlsl:141-149  total_weight > 0 is false for a NaN or a non-positive sum: blend_alpha stays 1, and
                              (1 - 1) * previous_color still adds 0 * previous_color (:159)
  preprocess.ps.hlsl:148      max(blend_alpha, BLEND_ALPHA): a NaN gives BLEND_ALPHA; postprocess.ps.hlsl:81 the same
  postprocess.ps.hlsl:41-42   in_prev_frame_pixel is RG16Float: int2() sees the rounded value
  regressionCP.hlsl:121-123   albedo < 0.01 ? 0 : noisy / albedo, so a NaN albedo divides
  regressionCP.hlsl:133-175   max / min drop a NaN operand: one NaN texel does not decide the block's range
  regressionCP.hlsl:260,268   vecLength > 0.01 and uLengthSquared < 0.001 are false for a NaN
  regressionCP.hlsl:496-499   x < 0 ? 0 : x keeps a NaN

MEASURED, LEFT_OUT and CAP at the end are printed by `python tests/test_edge_denoise_cpu.py` and asserted by the tests."""
import numpy as np

import bmfr_reference_numpy as ref
from edge_images import value_class
from test_bmfr_cross_check import FIT_RTOL, MARGIN, TEMPORAL_RTOL

F = np.float32
SIZES = ((7, 5), (33, 31), (40, 20), (65, 33))  # 40x20: narrower than a block offset; 65x33: two block columns
FRAMES = 4
# sample positions in the pixel, exact in float32; away from its centre, so that prev_frame_pixel_f = x + jitter - 0.5 of a
# still camera is no integer (and lies in (-0.5, 0) for some pixels of column or row 0)
JITTERS = ((0.25, 0.625), (0.75, 0.375), (0.375, 0.25), (0.625, 0.75))
# the camera's offset in pixels: moving (towards the corner that holds no special texel, so that the single texels on the
# bottom row and the right column keep reprojecting into the frame), then still
PANS = ((0, 0), (-1, 0), (-1, -1), (-1, -1))
OFFSET = 0.3125  # of the world origin from a pixel corner, in pixels: a background texel reprojects between pixel centres
FOOT = (1.0 / 32, 1.0 / 16)  # world units per pixel: a 32-pixel block spans < 1 in x (shifted only) and > 1 in y (scaled)

STAGES = {"pre": ref.PREPROCESS, "fit": ref.REGRESSION, "post": ref.POSTPROCESS, "temporal": ref.PREPROCESS | ref.POSTPROCESS,
          "all": ref.PREPROCESS | ref.REGRESSION | ref.POSTPROCESS}


def flag_sets():
    """(label, flags; a list: per frame): each stage alone, the two temporal ones and all three, half and full frame, both QR variants where the fit runs"""
    out = []
    for stage, bits in STAGES.items():
        for full in (0, ref.FULL_FRAME):
            for keep in ((0, ref.KEEP_LD_FEATURES) if bits & ref.REGRESSION else (0,)):
                out.append((f"{stage}/{'full' if full else 'half'}/{'keep_ld' if keep else 'ignore_ld'}", bits | full | keep))
    # flags that change from frame to frame: a frame without preprocess, and the half a half-frame call passes through,
    # put the caller's own noisy.w into the history that the next frame's preprocess reads (its sample_spp)
    every = STAGES["all"]
    for keep in (0, ref.KEEP_LD_FEATURES):
        name = "keep_ld" if keep else "ignore_ld"
        out.append((f"switch_stages/full/{name}", [b | ref.FULL_FRAME | keep for b in (STAGES["fit"], every, STAGES["fit"], every)]))
        out.append((f"switch_half/full/{name}", [every | f | keep for f in (0, ref.FULL_FRAME, 0, ref.FULL_FRAME)]))
    return out


def half(a):
    return np.asarray(a, F).astype(np.float16).astype(F)


HALF_BELOW = half(np.nextafter(np.float16(0.01), np.float16(0)))  # the largest half below 0.01 ...
HALF_ABOVE = half(0.01)                                           # ... and the smallest one >= 0.01
assert HALF_BELOW < F(0.01) <= HALF_ABOVE
HALF_SUBNORMAL = half(5 * 2.0 ** -24)
HALF_PATTERNS = np.array([0x7e00, 0x7c01, 0xfe00, 0x7c00, 0xfc00], np.uint16).view(np.float16).astype(F)  # NaNs and infs
NAN, INF = F(np.nan), F(np.inf)


# ---- where the special texels go ----------------------------------------------------------------------------------------
def places(W, H):
    """(singles [(x, y)], row y, block (bw, bh)): the block is x < bw, y < bh in the top left corner (the left half is
    what the half-frame mode processes), the row lies below it, the singles on the bottom row and the right column"""
    bw, bh = min(32, W - 2), min(32, H - 2)
    singles = []
    for t in range(max(W, H)):
        if t < W - 1:
            singles.append((t, H - 1))
        if t < H - 2:
            singles.append((W - 1, t))
    return singles, H - 2, (bw, bh)


def deal(W, H, k, count, size_index=0, singles_only=()):
    """variant number per texel of frame k as an [H, W] array, -1: ordinary.  singles_only: variants that sit on a
    decision's threshold by construction, where a float64 reading cannot follow a float32 implementation; they go to
    single pixels only, so that what the comparison leaves out stays under CAP"""
    singles, row, (bw, bh) = places(W, H)
    v = np.full((H, W), -1)
    wide = [i for i in range(count) if i not in singles_only]
    v[:bh, :bw] = wide[(k + size_index) % len(wide)]
    v[row, :] = wide[(k + size_index + 1) % len(wide)]
    step = max(1, len(singles) // (2 * count))
    for i, (x, y) in enumerate(singles[::step]):
        v[y, x] = (i + k) % count
    return v


# ---- the ordinary sequence ----------------------------------------------------------------------------------------------
def view_proj(W, H, k, mode):
    """prevViewProj of frame k (row-major, clip[r] = sum m[4r+c] * (pos, 1)[c]): maps a world point to where the camera
    of frame k-1 saw it.  'std': a screen translation over world units of FOOT per pixel, w = 1.  'ndc': world = NDC,
    identity (every value exact in float32).  'origin': a perspective camera whose eye is the origin looking down -z,
    the geometry at z = -3; a still camera."""
    m = np.zeros((4, 4))
    if k == 0 or mode == "ndc":
        return [float(v) for v in np.eye(4).ravel()]
    px, py = PANS[k - 1]
    sx, sy = 2.0 / (W * FOOT[0]), 2.0 / (H * FOOT[1])
    if mode == "origin":
        m[0, 0], m[1, 1], m[2, 2], m[3, 2] = 3 * sx, 3 * sy, 1.0, -1.0
    else:
        m[0, 0], m[1, 1], m[2, 2], m[3, 3] = sx, sy, 1.0, 1.0
        m[0, 3], m[1, 3] = 2.0 * (OFFSET - px) / W, -2.0 * (OFFSET - py) / H
    return [float(F(v)) for v in m.ravel()]


def ordinary(W, H, k, mode="std", seed=0):
    """Frame k of the ordinary sequence as a dict of [H, W, 4] float32 arrays (nrm and alb hold half values) and `vp`.
    A gently curved sheet around z = -3 ('origin': flat, so that the projection is the translation's), a normal that
    turns slowly, albedo in 0.2-0.8, a noisy colour = albedo * smooth irradiance * noise, spp 1."""
    rng = np.random.default_rng([W, H, k, seed])
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    jx, jy = JITTERS[k % 4]
    px, py = (0, 0) if mode in ("origin", "ndc") else PANS[k]
    if mode == "ndc":
        X, Y = 2 * (x + jx) / W - 1, 1 - 2 * (y + jy) / H
    else:
        off = 0.0 if mode == "origin" else OFFSET
        X, Y = (x + jx + px - W / 2 - off) * FOOT[0], (H / 2 - (y + jy + py) + off) * FOOT[1]
    Z = np.full_like(X, -3.0) if mode == "origin" else -3.0 + 0.1 * X - 0.05 * Y + 0.02 * X * Y
    pos = np.stack([X, Y, Z, np.ones_like(X)], -1)
    n = np.stack([-0.1 - 0.02 * Y, 0.05 - 0.02 * X, np.ones_like(X)], -1)
    nrm = np.concatenate([n / np.linalg.norm(n, axis=-1, keepdims=True), np.zeros((H, W, 1))], -1)
    alb = np.ones((H, W, 4))
    alb[..., :3] = 0.2 + 0.6 * rng.random((H, W, 3))
    irr = 0.5 + 0.3 * X[..., None] - 0.1 * Y[..., None] + 0.1 * nrm[..., 1:2]
    noisy = np.ones((H, W, 4))
    noisy[..., :3] = alb[..., :3] * irr * (1.0 + 0.3 * rng.standard_normal((H, W, 3)))
    return dict(pos=pos.astype(F), nrm=half(nrm), alb=half(alb), noisy=noisy.astype(F), prev_pos=None,
                vp=view_proj(W, H, k, mode))


def finish(frames):
    """[H, W, 4] -> [H*W, 4] contiguous float32"""
    for f in frames:
        for key in ("pos", "nrm", "alb", "noisy", "prev_pos"):
            if f[key] is not None:
                f[key] = np.ascontiguousarray(f[key], F).reshape(-1, 4)
    return frames


def apply_variants(frames, W, H, variants, size_index, singles_only=()):
    """variants: callables (frame, mask [H, W]) that rewrite the masked texels"""
    for k, f in enumerate(frames):
        v = deal(W, H, k, len(variants), size_index, singles_only)
        for i, fn in enumerate(variants):
            if (v == i).any():
                fn(f, v == i)
    return frames


def setter(key, value):
    """a variant that writes `value` (None: leave the component) into channel array `key` of the masked texels"""
    def fn(f, mask):
        for c, val in enumerate(value):
            if val is not None:
                f[key][mask, c] = val
    return fn


def both(*fns):
    def fn(f, mask):
        for g in fns:
            g(f, mask)
    return fn


BACKGROUND = both(setter("pos", (0, 0, 0, 0)), setter("nrm", (0, 0, 0, 0)))


# ---- families -----------------------------------------------------------------------------------------------------------
def _pf_of(c, size):
    """prev_frame_pixel_f of NDC coordinate c with the shader's float32 operations and an identity matrix
    (preprocess.ps.hlsl:64-78): ((c + 1) / 2) * size - 0.5"""
    u = (F(c) + F(1)) / F(2)
    return F(F(u * F(size)) - F(0.5))


def _search_pf(lo, hi, size):
    """(c, pf): a float32 NDC coordinate whose prev_frame_pixel_f lies in [lo, hi], or None.  (c + 1) / 2 has a
    granularity of 2^-25 near c = -1, so not every float32 pf can be reached: lo == hi asks for luck."""
    c = F(2.0 * ((lo + hi) / 2 + 0.5) / size - 1.0)
    down = up = c
    for _ in range(64):
        for cand in (down, up):
            if -1 <= cand <= 1 and F(lo) <= _pf_of(cand, size) <= F(hi):
                return F(cand), float(_pf_of(cand, size))
        down, up = np.nextafter(down, F(-2)), np.nextafter(up, F(2))
    return None


def _integer_pf(size, first):
    """an integer prev_frame_pixel_f >= first that float32 reaches exactly (there is one for every frame size used)"""
    for k in range(first, size - 1):
        hit = _search_pf(k, k, size)
        if hit:
            return hit
    raise AssertionError(size)


def border_cases(W, H):
    """((cx, pfx), (cy, pfy), tap): NDC coordinates, the prev_frame_pixel_f they land on and the one tap of the four to
    accept.  -0.5 is uv = 0; values in [-0.5, 0) truncate to 0 and leave a negative fraction (weights above 1 and below
    0); an integer leaves a zero weight; a value within 2^-10 below 4 rounds to 4 as a half, so that postprocess
    truncates to another pixel than preprocess did; (W-1, W-0.5] has its right-hand taps outside the frame; W-0.5 is
    uv = 1."""
    near = lambda t, size: _search_pf(t - 0.02, t + 0.02, size)
    zero_x = _search_pf(0.0, 0.0, W) or _search_pf(0.0, 2.0 ** -17, W)
    return [(near(-0.5, W) and _search_pf(-0.5, -0.5, W), _search_pf(-0.5, -0.5, H), 1),  # lone tap of weight -0.75
            (near(-0.25, W), _integer_pf(H, 1), 0), (near(-0.25, W), near(-0.25, H), 3), (near(-0.25, W), near(2.5, H), 1),
            (zero_x, near(1.25, H), 0), (_integer_pf(W, 2), _integer_pf(H, 2), 1),  # the accepted tap has weight 0
            # (tap 0: pixel 3 for preprocess; postprocess, which sees 4.0, reads pixel 4 with the whole weight)
            (_search_pf(4 - 2.0 ** -10 + 2.0 ** -14, 4 - 2.0 ** -14, W), near(1.5, H), 0),
            (near(1.5, W), _search_pf(4 - 2.0 ** -10 + 2.0 ** -14, 4 - 2.0 ** -14, H), 0),
            (near(W - 0.75, W), near(1.25, H), 0), (_search_pf(W - 0.5, W - 0.5, W), _search_pf(H - 0.5, H - 0.5, H), 0)]


def family_borders(W, H, size_index):
    """world = NDC and an identity prevViewProj: no rounding in the matrix product.  All texels of a case share one
    position, whose z is the case's own; the previous frame holds that position in the chosen tap's pixel and nowhere
    else."""
    frames = [ordinary(W, H, k, "ndc") for k in range(FRAMES)]
    cases = border_cases(W, H)
    points = [(cx, -cy, F(10 + i), F(1)) for i, ((cx, _), (cy, _), _) in enumerate(cases)]  # uy = (1 - c1) / 2
    for (_, (cy, pfy), _) in cases:
        assert F((F(1) - (-cy)) / F(2) * F(H)) - F(0.5) == F(pfy)
    variants = [both(setter("pos", p), setter("nrm", (0, 0, 1, 0))) for p in points]
    apply_variants(frames, W, H, variants, size_index, singles_only=(0, 1, 4, 5, 9))  # uv = 0 or 1, or an integer pf
    for f in frames[:-1]:  # the accepted tap's pixel of the previous frame, written last: it wins over a special texel
        for ((_, pfx), (_, pfy), tap), p in zip(cases, points):
            sx, sy = int(pfx) + (tap & 1), int(pfy) + (tap >> 1)
            if 0 <= sx < W and 0 <= sy < H:
                f["pos"][sy, sx] = p
                f["nrm"][sy, sx] = (0, 0, 1, 0)
    return {"borders": finish(frames)}


def family_background(W, H, size_index):
    """worldPosition (0,0,0,0) with a zero normal; 'origin': the previous camera sits there, so c = 0/0"""
    out = {}
    for mode, name in (("origin", "eye_at_origin"), ("std", "eye_elsewhere")):
        frames = [ordinary(W, H, k, mode) for k in range(FRAMES)]
        out[name] = finish(apply_variants(frames, W, H, [BACKGROUND], size_index))
    return out


def family_camera_plane(W, H, size_index):
    """the 'origin' camera: c[3] = -z.  z = +3 lies behind it and reprojects into [0,1] mirrored; z = +-0 with x != 0
    gives a +-inf quotient (outside); z = 0 = x gives 0/0"""
    frames = [ordinary(W, H, k, "origin") for k in range(FRAMES)]
    variants = [setter("pos", (None, None, 3.0, None)), setter("pos", (None, None, 0.0, None)),
                setter("pos", (None, None, -0.0, None)), setter("pos", (0.0, None, 0.0, None)),
                setter("pos", (-0.0, None, -0.0, None))]
    return {"camera_plane": finish(apply_variants(frames, W, H, variants, size_index))}


def _pd_steps():
    """float32 d with d*d the last float32 below 0.01f, and the next d (d*d >= 0.01f)"""
    d = F(np.sqrt(F(0.01)))
    while F(d * d) >= F(0.01):
        d = np.nextafter(d, F(0))
    while F(np.nextafter(d, F(1)) * np.nextafter(d, F(1))) < F(0.01):
        d = np.nextafter(d, F(1))
    return d, np.nextafter(d, F(1))


def family_thresholds(W, H, size_index):
    """a still 'ndc' camera on pixel centres + jitter; the special texels sit at z = 0 on one shared point and the
    previous frame holds, in the tap's pixel, that point moved along z by d with d*d one float32 step either side of
    0.01 (position_distance_squared, preprocess.ps.hlsl:116), or a normal whose squared distance is one half step
    either side of 1.0 (:128).  Second run: a block region whose z is -3.5 or -2.5 (block_max - block_min == 1.0,
    regressionCP.hlsl:179), and the same with -2.5 one float32 step nearer zero (> 1.0)."""
    d_in, d_out = _pd_steps()
    one_below, one_above = half(1 - 2.0 ** -11), half(1 + 2.0 ** -10)
    # (dz of the previous texel, its normal's x): the current normal is (0, 0, 1)
    cases = [(d_in, 0.0), (d_out, 0.0), (0.0, one_below), (0.0, 1.0), (0.0, one_above), (d_in, one_below)]
    frames = [ordinary(W, H, k, "ndc") for k in range(FRAMES)]
    spots = [(1.25, 1.5), (3.25, 0.5), (0.5, 2.25), (4.5, 1.25), (2.5, 3.25), (5.25, 2.5)]  # prev_frame_pixel_f per case
    hits = [(_search_pf(tx - 0.02, tx + 0.02, W), _search_pf(ty - 0.02, ty + 0.02, H)) for tx, ty in spots]
    points = [(hx[0], -hy[0], F(0), F(1)) for hx, hy in hits]
    variants = [both(setter("pos", p), setter("nrm", (0, 0, 1, 0))) for p in points]
    apply_variants(frames, W, H, variants, size_index, singles_only=(0, 1, 3, 5))  # on a limit, or one step from it
    for f in frames[:-1]:
        for (dz, nx), (tx, ty), p in zip(cases, spots, points):
            f["pos"][int(ty), int(tx)] = (p[0], p[1], dz, 1)
            f["nrm"][int(ty), int(tx)] = (nx, 0, 1, 0)
    out = {"taps": finish(frames)}
    frames = [ordinary(W, H, k) for k in range(FRAMES)]
    _, _, (bw, bh) = places(W, H)
    y, x = np.mgrid[0:H, 0:W]
    checker = ((x + y) % 2 == 0)
    for k, f in enumerate(frames):
        hi = F(-2.5) if k % 2 == 0 else np.nextafter(F(-2.5), F(0))
        f["pos"][:bh, :bw, 2] = np.where(checker[:bh, :bw], F(-3.5), hi)
    out["range"] = finish(frames)
    return out


def family_non_finite(W, H, size_index):
    """NaN, +-inf and subnormals in one component of position or normal; half NaN and inf patterns in the normal.  Two
    runs, because they spread differently: the rank-dropping QR drops a column that holds a NaN (regressionCP.hlsl:260)
    and leaves the NaN to its own texel, while an inf makes the column's norm inf and the whole block NaN."""
    nan = [setter("pos", (NAN, None, None, None)), setter("pos", (None, F(1e-40), None, None)),
           setter("nrm", (HALF_PATTERNS[0], None, None, None)), setter("nrm", (None, HALF_PATTERNS[1], None, None)),
           setter("nrm", (None, None, HALF_PATTERNS[2], None)), setter("nrm", (None, None, HALF_SUBNORMAL, None))]
    inf = [setter("pos", (None, INF, None, None)), setter("pos", (None, None, -INF, None)),
           setter("nrm", (HALF_PATTERNS[3], None, None, None)), setter("nrm", (None, HALF_PATTERNS[4], None, None))]
    out = {}
    for name, variants in (("nan", nan), ("inf", inf)):
        frames = [ordinary(W, H, k) for k in range(FRAMES)]
        out[name] = finish(apply_variants(frames, W, H, variants, size_index))
    return out


def family_huge(W, H, size_index):
    """+-1e30 in one component of the position: the squares overflow"""
    variants = [setter("pos", (F(1e30), None, None, None)), setter("pos", (None, None, F(-1e30), None))]
    frames = [ordinary(W, H, k) for k in range(FRAMES)]
    return {"huge": finish(apply_variants(frames, W, H, variants, size_index))}


def family_rank(W, H, size_index):
    """whole frames that leave the ten feature columns rank deficient, from frame 1 on: an axis-aligned flat wall (z and
    the normal constant); 1024 identical texels per block (every column constant; with KEEP_LD_FEATURES the R diagonal
    is feature noise only); y = 2x + c (two proportional columns, equal after scaling).  At 7x5 and 40x20 some blocks load
    nothing but texels outside the frame."""
    out = {}
    for name in ("wall", "identical", "proportional"):
        frames = [ordinary(W, H, k) for k in range(FRAMES)]
        for f in frames[1:]:
            if name == "wall":
                f["pos"][..., 2] = -3.0
                f["nrm"][...] = (0, 0, 1, 0)
            elif name == "identical":
                f["pos"][...] = (0.25, -0.5, -3.0, 1.0)
                f["nrm"][...] = (0, 0, 1, 0)
                f["alb"][...] = (0.5, 0.25, 0.75, 1.0)
            else:
                f["pos"][..., 1] = 2 * f["pos"][..., 0] + F(0.0137)  # (the shift keeps prev_frame_pixel_f off the integers)
        out[name] = finish(frames)
    return out


def _geometry(W, H, geometry, size_index):
    mode = "origin" if geometry == "background" else "std"
    frames = [ordinary(W, H, k, mode) for k in range(FRAMES)]
    if geometry == "background":  # (every other frame, so that a special colour meets both kinds of texel)
        apply_variants(frames, W, H, [BACKGROUND, lambda f, mask: None], size_index)
    return frames


ALBEDO_VARIANTS = [(HALF_BELOW, 0.5, 0.5, 1.0), (0.0, -0.0, -0.5, 0.0), (HALF_SUBNORMAL, 0.5, 0.5, 0.5),
                   (INF, 0.5, 0.5, 1.0), (0.5, NAN, 0.5, 1.0), (0.5, 0.5, 0.5, -1.0), (0.5, 0.5, 0.5, NAN),
                   (0.5, HALF_BELOW, 0.5, 0.0)]
# ill-conditioned: the smallest half >= 0.01 demodulates by 100 (regressionCP.hlsl:121-123), and the colour it divides is
# blended with the history of texels of ordinary albedo: a block holds demodulated colours of two scales.  And every
# albedo variant over background texels: those share one feature vector, so a fit isolates them, and where their
# demodulated colour is 0 (albedo < 0.01) it crosses zero there, where (0.01 + |r|) turns the ordinary float32 error of a
# fit into a large relative one (test_bmfr_cross_check.test_regression_clamps_negative_fits_at_zero leaves its scene out
# of the tolerance sweep for that reason)
ALBEDO_ILL_VARIANTS = [(HALF_BELOW, HALF_ABOVE, 0.5, 1.0), (0.5, 0.5, HALF_ABOVE, -1.0), (HALF_ABOVE, HALF_BELOW, 0.5, 0.0)]
# (the texels with a negative channel have a depth of their own, so that their taps are accepted among themselves only: a
# bilinear sum or a blend of both signs cancels, its error is of the size of its terms, and TEMPORAL_RTOL's absolute term is
# sized for sums of like sign)
COLOUR_VARIANTS = [(0.0, 0.0, 0.0, 1.0), both(setter("noisy", (-0.5, 0.3, 0.2, 1.0)), setter("pos", (None, None, 9.0, None))), (F(1e-40), 0.3, F(-1e-40), 1.0), (INF, 0.3, 0.2, 1.0),
                   (0.3, NAN, 0.2, 1.0), (0.3, 0.3, 0.3, 0.0), (0.3, 0.3, 0.3, NAN), (0.2, 0.3, -INF, 1.0),
                   # an incoming spp of -1 is the pole of blend_alpha = 1 / (sample_spp + 1) (preprocess.ps.hlsl:147), and
                   # one of 1e9 outweighs every tap beside it.  Both get a depth of their own, so that their taps are
                   # accepted among themselves only: sample_spp is then -1 or 1e9 exactly (beside taps of spp 1 it would
                   # be a cancelling sum, or a bilinear weight times 1e9, which float32 knows to 1e-5 of itself)
                   both(setter("noisy", (0.3, 0.3, 0.3, -1.0)), setter("pos", (None, None, 5.0, None))),
                   both(setter("noisy", (0.3, 0.3, 0.3, F(1e9))), setter("pos", (None, None, 7.0, None)))]
# ill-conditioned: 1e30 (sums of both signs cancel at that scale)
COLOUR_ILL_VARIANTS = [(F(1e30), 0.3, 0.2, 1.0), (0.3, F(-1e30), 0.2, 1.0)]


def _albedo_setter(value):
    """the albedo and, where a channel stays one the fit demodulates by (finite, >= 0.01), the noisy colour with it:
    radiance = albedo * irradiance, so that the demodulated colour keeps the scale of its neighbours'"""
    def fn(f, mask):
        for c, val in enumerate(value[:3]):
            if np.isfinite(val) and val >= F(0.01):
                f["noisy"][mask, c] = f["noisy"][mask, c] / f["alb"][mask, c] * F(val)
        setter("alb", value)(f, mask)
    return fn


BOTH = ("ordinary", "background")


def _colour_family(name, key, *runs):
    """runs: (variants, geometries): special values of `key` over ordinary geometry and / or over background texels"""
    def family(W, H, size_index):
        out = {}
        for i, (variants, geometries) in enumerate(runs):
            for geometry in geometries:
                frames = _geometry(W, H, geometry, size_index)
                apply_variants(frames, W, H, [v if callable(v) else _albedo_setter(v) if key == "alb" else setter(key, v)
                                              for v in variants], size_index)
                out[f"{geometry}{i if i else ''}"] = finish(frames)
        return out
    return family


def family_motion(W, H, size_index):
    """prev_pos (bdpt_bmfr_execute_motion): equal to the current position bit for bit, far away, NaN, and background"""
    frames = [ordinary(W, H, k) for k in range(FRAMES)]
    for f in frames:
        f["prev_pos"] = f["pos"].copy()
    variants = [setter("prev_pos", (None, None, None, None)), lambda f, m: f["prev_pos"].__setitem__(m, f["pos"][m] + F(100)),
                setter("prev_pos", (NAN, None, None, None)), setter("prev_pos", (0, 0, 0, 0)),
                both(setter("prev_pos", (0, 0, 0, 0)), BACKGROUND)]
    out = {"moved": finish(apply_variants(frames, W, H, variants, size_index))}
    frames = [ordinary(W, H, k) for k in range(FRAMES)]
    for f in frames:
        f["prev_pos"] = f["pos"].copy()
    out["unmoved"] = finish(frames)
    return out


FAMILIES = {
    "background": family_background, "camera_plane": family_camera_plane, "borders": family_borders,
    "thresholds": family_thresholds, "non_finite": family_non_finite, "huge": family_huge, "rank": family_rank,
    "albedo": _colour_family("albedo", "alb", (ALBEDO_VARIANTS, ("ordinary",))),
    "albedo_ill": _colour_family("albedo_ill", "alb", (ALBEDO_ILL_VARIANTS, BOTH), (ALBEDO_VARIANTS, ("background",))),
    "colour": _colour_family("colour", "noisy", (COLOUR_VARIANTS, BOTH)),
    "colour_ill": _colour_family("colour_ill", "noisy", (COLOUR_ILL_VARIANTS, BOTH)), "motion": family_motion,
}
# ill-conditioned by construction: their fits are compared with the bound measured for them (MEASURED), not FIT_RTOL
ILL = ("rank", "huge", "albedo_ill", "colour_ill")
WELL = tuple(n for n in FAMILIES if n not in ILL)


# thresholds/range is about the fit's scaling decision.  Its checkerboard of depths also leaves preprocess two diagonal taps
# of contrasting colours, whose blend follows the bilinear weights' float32 error (the fraction of a prev_frame_pixel_f of
# up to 65) beyond TEMPORAL_RTOL: it runs the flag sets of the fit alone.
ONLY_STAGE = {("thresholds", "range"): "fit"}


def sequences(family, W, H):
    """{run name: [frame dicts]} of a family at one frame size"""
    return FAMILIES[family](W, H, SIZES.index((W, H)))


def flag_sets_of(family, run):
    stage = ONLY_STAGE.get((family, run))
    return [(label, flags) for label, flags in flag_sets() if stage is None or label.startswith(stage + "/")]


def params(pkg, k, flags, vp):
    p = pkg.abi.BmfrParams()
    p.frameNumber, p.flags = k, flags
    for i in range(16):
        p.prevViewProj[i] = vp[i]
    return p


# ---- the comparison with the reading --------------------------------------------------------------------------------------
def broad_class(a):
    """edge_images.value_class with zero and finite as one class and their sign left to the numeric comparison: a clamp
    at zero, an underflow or a cancellation turns a small float64 into a float32 zero of either sign"""
    c = value_class(np.asarray(a, np.float64).astype(F))
    return np.where((c & 3) <= 1, 1, c)


class Tally:
    """what one family's comparisons saw: worst errors, texels compared and left out"""

    def __init__(self):
        self.fit = {False: 0.0, True: 0.0}  # by KEEP_LD_FEATURES
        self.temporal = 0.0
        self.written = self.left_out = self.classes = self.nonfinite = 0
        self.causes = {"pre": 0, "fit": 0, "post": 0}  # left out by stage (a texel may count under several)
        self.bad = []
        self.worst = {}  # where the worst errors were: (label, got, want)

    def merge(self, other):
        for key in self.fit:
            if other.fit[key] > self.fit[key]:
                self.fit[key], self.worst[key] = other.fit[key], other.worst.get(key)
        if other.temporal > self.temporal:
            self.temporal, self.worst["temporal"] = other.temporal, other.worst.get("temporal")
        for name in ("written", "left_out", "classes", "nonfinite"):
            setattr(self, name, getattr(self, name) + getattr(other, name))
        for key in self.causes:
            self.causes[key] += other.causes[key]
        self.bad += other.bad


def _compare(tally, label, got, want, ok, kind, keep_ld=False, scale=None):
    """got (float32) against want (float64) on the texels `ok`: classes first, then the finite values.  kind 'temporal':
    (|g - w| - 1e-7) / |w|, to be held to TEMPORAL_RTOL (test_bmfr_cross_check.temporal_close's rule); 'fit':
    |g - w| / (0.01 + |w|), or with `scale` (ILL families) / (0.01 + the frame's largest finite |w|)."""
    g, w = got[ok].astype(np.float64), want[ok]
    cg, cw = broad_class(g), broad_class(w)
    if not np.array_equal(cg, cw):
        tally.bad.append(f"{label}: {int((cg != cw).sum())} values of another class (got {cg[cg != cw][:4]}, want {cw[cg != cw][:4]})")
    tally.classes += g.size
    fin = (cg == 1) & (cw == 1)
    tally.nonfinite += int((cw != 1).sum())
    if not fin.any():
        return
    w32 = w[fin].astype(F).astype(np.float64)  # (an overflow or underflow of the float32 result is the class's business)
    d = np.abs(g[fin] - w32)
    if kind == "temporal":
        e = np.maximum(d - 1e-7, 0) / np.maximum(np.abs(w32), 1e-30)
        if e.max() > tally.temporal:
            tally.temporal, i = float(e.max()), int(e.argmax())
            tally.worst["temporal"] = (label, float(g[fin][i]), float(w32[i]))
    else:
        e = d / (0.01 + (np.abs(w32) if scale is None else scale))
        if e.max() > tally.fit[keep_ld]:
            tally.fit[keep_ld], i = float(e.max()), int(e.argmax())
            tally.worst[keep_ld] = (label, float(g[fin][i]), float(w32[i]))


def check_frame(tally, label, W, H, k, flags, f, history, out, state, sem=ref.D3D, ill=False):
    """One frame of an implementation against the reading, which starts from the implementation's own history
    (`history`: dict of prev_pos, prev_norm, prev_noisy, prev_filtered, accept, prev_pixel as the implementation left
    them), so that each frame is checked on its own and nothing left out spreads.  out: the implementation's image after
    the call; state: its (prev_noisy, accept, prev_pixel) after the call.  Texels whose decisions have a margin below
    MARGIN are left out and counted; where only the RG16Float store of prev_frame_pixel_f is within MARGIN of a rounding
    tie the implementation's value must be one of the two candidates, and the reading goes on with it."""
    n = W * H
    S = ref.State(W, H)
    with np.errstate(invalid="ignore"):  # (widening a signalling NaN)
        for key, val in history.items():
            setattr(S, key, np.array(val, np.float64 if key != "accept" else np.uint32))
    x = np.arange(n) % W
    proc = np.ones(n, bool) if flags & ref.FULL_FRAME else ~((x + 0.5) / W > 0.5)
    keep_ld = bool(flags & ref.KEEP_LD_FEATURES)
    with np.errstate(invalid="ignore"):
        pos, nrm, alb, noisy = (np.asarray(f[key], np.float64) for key in ("pos", "nrm", "alb", "noisy"))
    o_noisy, o_accept, o_pixel = state
    bad = np.zeros(n, bool)
    cur = noisy
    if flags & ref.PREPROCESS:
        cur, m_pre, _ = ref.preprocess(S, k, flags, f["vp"], pos, nrm, noisy, f["prev_pos"], sem)
        bad = proc & (m_pre < MARGIN)
        ok = proc & ~bad
        if not np.array_equal(o_accept[ok], S.accept[ok]):
            tally.bad.append(f"{label}: accept differs at {int((o_accept[ok] != S.accept[ok]).sum())} texels")
        _compare(tally, label + " preprocess", o_noisy, cur, ok, "temporal")
        if not np.array_equal(o_noisy[~proc].view(np.uint32), f["noisy"][~proc].view(np.uint32)):
            tally.bad.append(f"{label}: preprocess touched the half it passes through")
        if k > 0:
            pix_ok = ok & S.diag["inside"]
            amb = pix_ok & (S.diag["half_margin"] < MARGIN)
            sure = pix_ok & ~amb
            pc, oc = S.prev_pixel[sure], o_pixel[sure].astype(np.float64)
            if not ((pc == oc) | (np.isnan(pc) & np.isnan(oc))).all():
                tally.bad.append(f"{label}: prev_frame_pixel_f differs at {int(((pc != oc) & ~(np.isnan(pc) & np.isnan(oc))).any(1).sum())} texels")
            pf = S.diag["pf"][amb]
            h = pf.astype(np.float16)
            step = np.maximum(np.nextafter(h, np.float16(np.inf)) - h, h - np.nextafter(h, np.float16(-np.inf))).astype(np.float64)
            oa = o_pixel[amb].astype(np.float64)
            # one float16 step, or the margin's window where the steps are finer than that (near 0)
            if not (np.abs(oa - h) <= np.maximum(step, MARGIN * np.maximum(1.0, np.abs(pf)))).all():
                tally.bad.append(f"{label}: an ambiguous prev_frame_pixel_f is neither candidate")
            S.prev_pixel[amb] = o_pixel[amb]
        S.accept[bad], S.prev_pixel[bad] = o_accept[bad], o_pixel[bad]
    tally.written += int(proc.sum())
    tally.causes["pre"] += int(bad.sum())
    S.prev_noisy = o_noisy.astype(np.float64)  # the blit; the implementation's, so that the fit reads what it read
    final_bad = bad.copy()
    if flags & ref.REGRESSION:
        cur, m_fit = ref.fit(W, H, k, flags, pos, nrm, alb, S.prev_noisy, sem=sem)
        final_bad |= m_fit < MARGIN
        tally.causes["fit"] += int((m_fit < MARGIN).sum())
    else:
        cur = S.prev_noisy
    if flags & ref.POSTPROCESS:
        cur, m_post, _ = ref.postprocess(S, k, flags, cur, sem)
        final_bad |= proc & (m_post < MARGIN)
        tally.causes["post"] += int((proc & (m_post < MARGIN)).sum())
    if flags & (ref.REGRESSION | ref.POSTPROCESS):
        ok = ~final_bad
        kind = "fit" if flags & ref.REGRESSION else "temporal"
        scale = None
        if ill and kind == "fit":
            finite = np.abs(cur[:, :3][np.isfinite(cur[:, :3])])
            scale = float(finite.max()) if finite.size else 0.0
        _compare(tally, label + " rgb", out[:, :3], cur[:, :3], ok, kind, keep_ld, scale)
        w_want = cur[:, 3].astype(F)
        same = (out[ok, 3] == w_want[ok]) | (np.isnan(out[ok, 3]) & np.isnan(w_want[ok]))
        if not same.all():
            tally.bad.append(f"{label}: w differs at {int((~same).sum())} texels")
    tally.left_out += int((final_bad & (proc | bool(flags & ref.REGRESSION))).sum())


def run_sequence(tally, label, pkg, W, H, flags, frames, execute, sem=ref.D3D, ill=False):
    """execute(k, params, frame) -> (out, (prev_noisy, accept, prev_pixel)) of an implementation that keeps its own
    history; every frame is checked with check_frame"""
    n = W * H
    hist = dict(prev_pos=np.zeros((n, 4)), prev_norm=np.zeros((n, 4)), prev_noisy=np.zeros((n, 4)), prev_filtered=np.zeros((n, 4)),
                accept=np.zeros(n, np.uint32), prev_pixel=np.zeros((n, 2)))
    for k, f in enumerate(frames):
        fl = flags[k] if isinstance(flags, list) else flags
        out, state = execute(k, params(pkg, k, fl, f["vp"]), f)
        check_frame(tally, f"{label} frame {k}", W, H, k, fl, f, hist, out, state, sem, ill)
        hist["prev_pos"], hist["prev_norm"], hist["prev_noisy"] = f["pos"], f["nrm"], state[0]
        hist["accept"], hist["prev_pixel"] = state[1], state[2]
        if fl & ref.POSTPROCESS:
            hist["prev_filtered"] = out


def oracle_executor(pkg, ob, W, H):
    b = ob.OracleBmfr(pkg.abi, W, H)

    def execute(k, p, f):
        out = f["noisy"].copy()
        b.execute(p, f["pos"], f["nrm"], f["alb"], out, f["prev_pos"])
        return out, b.state()
    return b, execute


# ---- measured tables (printed by `python tests/test_edge_denoise_cpu.py`) -------------------------------------------------
# Worst deviation of the oracle from the reading per family over every size, run, flag set and frame: `fit` as _compare's
# 'fit' (by KEEP_LD_FEATURES), `temporal` as its 'temporal'.  The WELL families are held to FIT_RTOL / TEMPORAL_RTOL;
# the ILL ones to ten times what is recorded here (the margin FIT_RTOL documents), their fits relative to the frame's
# largest finite value.
MEASURED = {
    "background": {"fit": {False: 5.3e-05, True: 3.9e-06}, "temporal": 3.8e-06},
    "camera_plane": {"fit": {False: 4.7e-05, True: 1.6e-06}, "temporal": 3.8e-06},
    "borders": {"fit": {False: 4.4e-05, True: 3.2e-06}, "temporal": 2.9e-06},
    "thresholds": {"fit": {False: 3.7e-04, True: 4.7e-06}, "temporal": 2.9e-06},
    "non_finite": {"fit": {False: 3.1e-05, True: 8.7e-07}, "temporal": 3.7e-06},
    "huge": {"fit": {False: 2.0e-05, True: 0.0e+00}, "temporal": 3.7e-06},
    "rank": {"fit": {False: 4.4e-05, True: 9.3e-07}, "temporal": 8.5e-06},
    "albedo": {"fit": {False: 1.9e-04, True: 3.9e-06}, "temporal": 3.7e-06},
    "albedo_ill": {"fit": {False: 2.3e-04, True: 9.3e-06}, "temporal": 6.3e-06},
    "colour": {"fit": {False: 1.2e-04, True: 2.1e-06}, "temporal": 5.0e-06},
    "colour_ill": {"fit": {False: 1.1e-04, True: 3.4e-06}, "temporal": 2.6e-05},
    "motion": {"fit": {False: 2.5e-04, True: 6.7e-06}, "temporal": 3.7e-06},
}
# texels left out of a comparison (a decision inside MARGIN) of the texels a call processes, per family; CAP: 2 %
LEFT_OUT = {
    "background": {"left_out": 0, "of": 450544},  # 0.00 %
    "camera_plane": {"left_out": 0, "of": 225272},  # 0.00 %
    "borders": {"left_out": 1156, "of": 225272},  # 0.51 %
    "thresholds": {"left_out": 896, "of": 273584},  # 0.33 %
    "non_finite": {"left_out": 0, "of": 450544},  # 0.00 %
    "huge": {"left_out": 0, "of": 225272},  # 0.00 %
    "rank": {"left_out": 48, "of": 675816},  # 0.01 %
    "albedo": {"left_out": 8, "of": 225272},  # 0.00 %
    "albedo_ill": {"left_out": 11934, "of": 675816},  # 1.77 %
    "colour": {"left_out": 28, "of": 450544},  # 0.01 %
    "colour_ill": {"left_out": 0, "of": 450544},  # 0.00 %
    "motion": {"left_out": 8, "of": 450544},  # 0.00 %
}
CAP = 0.02
