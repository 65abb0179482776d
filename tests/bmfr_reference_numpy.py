"""A second, independent reading of the reference's BMFR denoise pass in float64 numpy, used only to cross-check the
oracle (tests/test_bmfr_cross_check.py) and, through it, the HIP kernels.  Written from the shaders, not from the
oracle; one function per stage:

  execute          BidirectionalPathtracing/Passes/DenoisePass.cpp:146-204   stage order and blits
  preprocess       BidirectionalPathtracing/Data/preprocess.ps.hlsl:33-165  temporal reprojection of the noisy frame
  fit              BidirectionalPathtracing/Data/regressionCP.hlsl:100-500  blockwise feature regression
                   (dispatch size: DenoisePass.cpp:250-270)
  postprocess      BidirectionalPathtracing/Data/postprocess.ps.hlsl:22-91  temporal accumulation of the filtered frame

The regression fits the albedo-demodulated colour to ten features per 32x32 block.  With feature noise
(KEEP_LD_FEATURES) that is a plain least-squares fit, solved here by np.linalg.lstsq.  The default variant drops
columns and may skip reflections, so there the reading replays the Householder pass in float64 and solves the
triangular system with np.linalg.solve.  Every discrete decision reports its margin, relative to the
quantity it compares, so that a test can leave out the elements an fp32 rounding could send the other way.

Non-finite values follow D3D (tests/edge_denoise.py feeds them): max / min return the operand that is not a NaN
(preprocess.ps.hlsl:148, postprocess.ps.hlsl:81, regressionCP.hlsl:133-175), int() of a NaN is 0 and saturates
(preprocess.ps.hlsl:80, postprocess.ps.hlsl:42), a load outside a texture is 0.  A least-squares problem with a
non-finite entry has no solution: its weights are NaN.  `Semantics` switches each of these to what C++ or x86 would
do instead, for the tests that show the comparison can tell.
"""
import numpy as np

PREPROCESS, REGRESSION, POSTPROCESS, KEEP_LD_FEATURES, FULL_FRAME = 1, 2, 4, 8, 16  # include/bdpt.h BDPT_BMFR_*

BUFFER_COUNT, FEATURES, FEATURES_NOT_SCALED, BLOCK_PIXELS, BLOCK_EDGE = 13, 10, 4, 1024, 32  # regressionCP.hlsl:27-33
NOISE_AMOUNT = 0.01
# BLOCK_OFFSETS, regressionCP.hlsl:38-56
BLOCK_OFFSETS = np.array([(-30, -30), (-12, -22), (-24, -2), (-8, -16), (-26, -24), (-14, -4), (-4, -28), (-26, -16),
                          (-4, -2), (-24, -32), (-10, -10), (-18, -18), (-12, -30), (-32, -4), (-2, -20), (-22, -12)])
POSITION_LIMIT_SQUARED, NORMAL_LIMIT_SQUARED, BLEND_ALPHA = 0.01, 1.0, 0.2  # preprocess.ps.hlsl:19-21
SECOND_BLEND_ALPHA = 0.1  # postprocess.ps.hlsl:5
RANK_LIMIT, U_LENGTH_LIMIT = 0.01, 0.001  # regressionCP.hlsl:260, 268


class Semantics:
    """How the reading treats what C++ leaves open.  The defaults are D3D's."""

    def __init__(self, max_keeps_nan=False, int_of_nan=0, round_prev_pixel=True):
        self.max_keeps_nan = max_keeps_nan        # True: std::max / std::min, a NaN operand stays
        self.int_of_nan = int_of_nan              # -2**31: what cvttss2si gives
        self.round_prev_pixel = round_prev_pixel  # False: prev_frame_pixel_f kept as computed, not as RG16Float holds it


D3D = Semantics()


def d3d_max(a, b, sem=D3D):
    return np.where(np.isnan(a) | np.isnan(b), np.nan, np.maximum(a, b)) if sem.max_keeps_nan else np.fmax(a, b)


def d3d_int(v, sem=D3D):
    """ftoi: toward zero, NaN -> 0, saturating at the ends of int32."""
    nan = np.isnan(v)
    t = np.clip(np.trunc(np.where(nan, 0.0, v)), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)
    return np.where(nan, np.int64(sem.int_of_nan), t)


def _no_nan(margin):
    """a comparison with a NaN is false at every precision: no rounding can send it the other way"""
    return np.where(np.isnan(margin), np.inf, margin)


def _inf_blend_margin(blend, cur, prev):
    """an infinite blend_alpha (1 / 0: an spp of -1 or 0) makes blend * cur + (1 - blend) * prev an inf or a NaN by the
    signs of cur and prev alone: each sign is a decision, with the operand's size as its margin"""
    small = np.minimum(np.abs(cur), np.abs(prev)).min(axis=1)
    return np.where(np.isinf(blend), _no_nan(small), np.inf)


def _back_substitute(R, Y):
    """R w = Y for upper-triangular R, last row first (regressionCP.hlsl:332-352): a non-finite entry reaches the
    weights the shader's order lets it reach."""
    k = R.shape[0]
    w = np.zeros_like(Y)
    Y = Y.copy()
    for i in range(k - 1, -1, -1):
        w[i] = Y[i] / R[i, i]
        Y[:i] -= R[:i, i:i + 1] * w[i][None, :]
    return w


def dispatch_blocks(W, H, full):
    """DenoisePass.cpp:255-262: ((W+31)/32 + 1) x ((H+31)/32 + 1) blocks; the reference halves the width in blocks
    (it filters the left half only); FULL_FRAME keeps the whole width."""
    w, h = (W + 31) // 32 + 1, (H + 31) // 32 + 1
    return (w if full else w // 2), h


def block_offset(frame):
    """frame_number is a uint in the constant buffer (regressionCP.hlsl:3), so frame_number % 16 is unsigned."""
    return BLOCK_OFFSETS[(int(frame) & 0xFFFFFFFF) % 16]


def _hash(a):
    """random(uint), regressionCP.hlsl:75-84, on uint32 arrays (wraparound), then float(a) / 2^32: float(a) rounds the
    uint to fp32 first, which we keep (an exact power-of-two divide follows)."""
    a = a.astype(np.uint32)
    with np.errstate(over="ignore"):
        a = (a + np.uint32(0x7ed55d16)) + (a << np.uint32(12))
        a = (a ^ np.uint32(0xc761c23c)) ^ (a >> np.uint32(19))
        a = (a + np.uint32(0x165667b1)) + (a << np.uint32(5))
        a = (a + np.uint32(0xd3a2646c)) ^ (a << np.uint32(9))
        a = (a + np.uint32(0xfd7046c5)) + (a << np.uint32(3))
        a = (a ^ np.uint32(0xb55a4f09)) ^ (a >> np.uint32(16))
    return a.astype(np.float32).astype(np.float64) / 4294967296.0


def feature_noise(frame):
    """add_random (regressionCP.hlsl:86-95) for every in-block pixel and feature column: [1024, 10], column 0 zero.
    The shader sums id + sub*256 + buffer*1024 + frame*13312 in int and hands it to random(uint): 32-bit wraparound.
    id + sub*256 is the in-block pixel index."""
    idx = np.arange(BLOCK_PIXELS, dtype=np.int64)[:, None] + np.arange(FEATURES, dtype=np.int64)[None, :] * 1024
    arg = (idx + (int(frame) & 0xFFFFFFFF) * (BUFFER_COUNT * BLOCK_EDGE * BLOCK_EDGE)) & 0xFFFFFFFF
    noise = NOISE_AMOUNT * 2 * (_hash(arg) - 0.5)
    noise[:, 0] = 0.0
    return noise


def _mirror(i, size):
    """mirror(), regressionCP.hlsl:58-66: one reflection only."""
    return np.where(i < 0, -i - 1, np.where(i >= size, 2 * size - i - 1, i))


def _fit_ignore_ld(F, Y):
    """IGNORE_LD_fEATURES (regressionCP.hlsl:200-355) in float64: Householder over the feature columns in order.  A
    column is kept when the norm of what the kept columns leave of it (rows limit.. after their reflections) exceeds
    0.01, else its weight is 0.  A kept column whose reflector u has |u|^2 < 0.001 gets its R entries (the column
    above the pivot, the norm on it) but its reflection is not applied to the columns after it nor to the colour.
    Then R w = (Q^T Y) over the kept rows, solved by np.linalg.solve.  Returns (w [10, 3], margin): the smallest of
    |norm - 0.01| / 0.01 and |(|u|^2 - 0.001)| / 0.001 over the columns."""
    M = np.concatenate([F, Y], axis=1)
    R = np.zeros((FEATURES, FEATURES))
    limit, kept, margin = 0, [], np.inf
    for col in range(FEATURES):
        x = M[limit:, col]
        vec_length = float(np.sqrt(x @ x))
        if not np.isnan(vec_length):
            margin = min(margin, abs(vec_length - RANK_LIMIT) / RANK_LIMIT)
        if not vec_length > RANK_LIMIT:
            continue
        R[:limit, len(kept)] = M[:limit, col]
        R[limit, len(kept)] = vec_length
        kept.append(col)
        u = x.copy()
        u[0] -= vec_length
        uls = float(u @ u)
        if not np.isnan(uls):
            margin = min(margin, abs(uls - U_LENGTH_LIMIT) / U_LENGTH_LIMIT)
        if not uls < U_LENGTH_LIMIT:
            M[limit:, col + 1:] -= np.outer(u, 2.0 * (u @ M[limit:, col + 1:]) / uls)
        limit += 1
    w = np.zeros((FEATURES, 3))
    k = len(kept)
    if np.isfinite(R[:k, :k]).all() and np.isfinite(M[:k, FEATURES:]).all():
        w[kept] = np.linalg.solve(R[:k, :k], M[:k, FEATURES:])
    else:
        w[kept] = _back_substitute(R[:k, :k], M[:k, FEATURES:])
    return w, margin


def fit(W, H, frame, flags, pos, nrm, alb, noisy, offset_frame=None, clamp=True, sem=D3D):
    """regressionCP.hlsl fit() over the whole dispatch.  pos / nrm / alb / noisy: [H*W, 4] (nrm and alb already
    half-decoded); `noisy` is the copy of gCurNoisy blitted to BMFR_PrevNoisy just before the dispatch
    (DenoisePass.cpp:180), which is what every mirrored load reads.  Returns (out [H*W, 4] float64, margin [H*W]):
    out holds `noisy` where no block writes; margin is the smallest decision margin of the block that wrote a pixel
    (inf where none did).  offset_frame: take the block offset of that frame instead (a deliberately wrong reading,
    for the test that the comparison can tell).  clamp=False: leave negative fits as they are (for a test of the
    clamp)."""
    full = bool(flags & FULL_FRAME)
    keep_ld = bool(flags & KEEP_LD_FEATURES)
    pos, nrm, alb, noisy = (np.asarray(a, np.float64).reshape(H * W, 4) for a in (pos, nrm, alb, noisy))
    out = noisy.copy()
    margin = np.full(H * W, np.inf)
    bw, bh = dispatch_blocks(W, H, full)
    ox, oy = block_offset(frame if offset_frame is None else offset_frame)
    index = np.arange(BLOCK_PIXELS)
    noise = feature_noise(frame) if keep_ld else None
    for g in range(bw * bh):
        # uv of each in-block pixel (regressionCP.hlsl:104-108), then its mirrored load position (:109)
        ux = (g % bw) * BLOCK_EDGE + index % BLOCK_EDGE + ox
        uy = (g // bw) * BLOCK_EDGE + index // BLOCK_EDGE + oy
        mx, my = _mirror(ux, W), _mirror(uy, H)
        # a frame narrower than an offset is not covered by one reflection: those loads leave the texture and return 0
        inside = (mx >= 0) & (my >= 0) & (mx < W) & (my < H)
        li = np.where(inside, my * W + mx, 0)
        P = np.where(inside[:, None], pos[li, :3], 0.0)
        N = np.where(inside[:, None], nrm[li, :3], 0.0)
        A = np.where(inside[:, None], alb[li, :3], 0.0)
        C = np.where(inside[:, None], noisy[li, :3], 0.0)
        # features (:110-119): 1, normal, position, position squared; colour demodulated by albedo (>= 0.01 only).
        # tmp_data is an R32Float texture (:12): a feature is what fp32 holds of it, which matters for a square near
        # 1e8 (its fp32 rounding is of the order of what a block's linear fit leaves of it)
        with np.errstate(all="ignore"):
            F = np.concatenate([np.ones((BLOCK_PIXELS, 1)), N, P, (P * P).astype(np.float32)], axis=1)
            Y = np.where(A < 0.01, 0.0, C / np.where(A < 0.01, 1.0, A))
        # features 4..9 scaled by the block's range when it exceeds 1, else only shifted (:122-182)
        m = np.finfo(np.float64).max  # (finite: an infinite margin marks the pixels no block writes)
        for fb in range(FEATURES_NOT_SCALED, FEATURES):
            # max / min drop a NaN operand (D3D), so one NaN texel does not decide the block's range
            col = F[:, fb]
            if sem.max_keeps_nan:
                lo, hi = col.min(), col.max()
            else:
                lo, hi = np.fmin.reduce(col), np.fmax.reduce(col)
            with np.errstate(all="ignore"):
                # the features are R32Float texels, so hi - lo here is exact and the shader's block_max - block_min
                # (:179) is its one rounding: the reading takes the shader's decision, and no margin is needed
                wide = np.float32(hi - lo) > 1.0
                F[:, fb] = ((col - lo) / (hi - lo) if wide else col - lo).astype(np.float32)  # R32Float
        with np.errstate(all="ignore"):
            if keep_ld:
                # plain Householder QR (:331-440): the noise goes into the copy being factorised only (columns 1-9, at
                # col == 0, before the first reflection touches them); the colour columns stay noise-free.  A
                # non-finite feature leaves no least-squares problem for any channel, a non-finite colour none for its
                # own channel
                w = np.full((FEATURES, 3), np.nan)
                if np.isfinite(F).all():
                    for ch in range(3):
                        if np.isfinite(Y[:, ch]).all():
                            w[:, ch] = np.linalg.lstsq(F + noise, Y[:, ch], rcond=None)[0]
            else:
                w, rank_m = _fit_ignore_ld(F, Y)
                m = min(m, rank_m)
            # filtered colour on the noise-free features (:458-475), clamped at 0 (r < 0 ? 0 : r: a NaN stays) and
            # re-modulated by albedo; only pixels that were not mirrored are written (:477-498)
            fitted = (F[:, :, None] * w[None, :, :]).sum(axis=1) if not (np.isfinite(F).all() and np.isfinite(w).all()) else F @ w
            if clamp:
                fitted = np.where(fitted < 0.0, 0.0, fitted)
            write = (ux >= 0) & (uy >= 0) & (ux < W) & (uy < H)
            oi = (uy * W + ux)[write]
            out[oi, :3] = alb[oi, :3] * fitted[write]
            out[oi, 3] = alb[oi, 3] * noisy[oi, 3]  # exact in float64; rounds to the fp32 product
        margin[oi] = m
    return out, margin


def _trunc_margin(v):
    """int() truncates toward zero: discontinuous at every non-zero integer (not at 0)."""
    r = np.round(v)
    r = np.where(r == 0, np.sign(v) + (v == 0), r)  # nearest non-zero integer
    return np.abs(v - r) / np.maximum(1.0, np.abs(v))


def _half_margin(v):
    """RG16Float store: distance to the nearest float16 rounding midpoint, relative to max(1, |v|)."""
    h = v.astype(np.float16)
    up = np.nextafter(h, np.float16(np.inf)).astype(np.float64)
    dn = np.nextafter(h, np.float16(-np.inf)).astype(np.float64)
    hf = h.astype(np.float64)
    d = np.minimum(np.abs(v - (hf + up) / 2), np.abs(v - (hf + dn) / 2))
    return d / np.maximum(1.0, np.abs(v))


TAPS = ((0, 0), (1, 0), (0, 1), (1, 1))


class State:
    """The pass's textures that cross frames (DenoisePass.h): BMFR_PrevPos / PrevNorm / PrevNoisy / PrevFiltered,
    BMFR_AcceptedBools, BMFR_PrevFramePixel (RG16Float, kept as the float16 values)."""

    def __init__(self, W, H):
        self.W, self.H = W, H
        n = W * H
        self.prev_pos = np.zeros((n, 4))
        self.prev_norm = np.zeros((n, 4))
        self.prev_noisy = np.zeros((n, 4))
        self.prev_filtered = np.zeros((n, 4))
        self.accept = np.zeros(n, np.uint32)
        self.prev_pixel = np.zeros((n, 2))


def preprocess(S, frame, flags, view_proj, pos, nrm, noisy, prev_pos=None, sem=D3D):
    with np.errstate(all="ignore"):  # non-finite inputs are part of the job
        return _preprocess(S, frame, flags, view_proj, pos, nrm, noisy, prev_pos, sem)


def _preprocess(S, frame, flags, view_proj, pos, nrm, noisy, prev_pos, sem):
    """preprocess.ps.hlsl main() for every pixel.  view_proj: prevViewProjMat as 16 floats, row-major in the ABI's
    sense (clip[r] = sum_c m[4r+c] * (pos, 1)[c]).  Updates S.accept / S.prev_pixel.  Returns (out [n,4],
    margin [n], taps [n,4]): taps are the history pixels whose colour went into each result (-1: none).  prev_pos
    (bdpt_bmfr_execute_motion): where each pixel's surface point was in the previous frame; it is what is reprojected
    and what the taps' positions are compared with."""
    W, H = S.W, S.H
    n = W * H
    x, y = np.arange(n) % W, np.arange(n) // W
    out = noisy.copy()
    margin = np.full(n, np.inf)
    taps = np.full((n, 4), -1)
    # texC.x > 0.5 returns the noisy colour untouched, and writes neither accept_bools nor out_prev_frame_pixel
    proc = np.ones(n, bool) if flags & FULL_FRAME else ~((x + 0.5) / W > 0.5)
    cur = noisy[:, :3]
    if frame == 0:
        pf = np.stack([x + 0.5, y + 0.5], axis=1)  # prev_frame_pixel_f defaults to pos.xy
        out[proc, 3] = 1.0
        S.accept[proc] = 0
        S.prev_pixel[proc] = pf[proc].astype(np.float16).astype(np.float64)
        return out, margin, taps
    m = np.asarray(view_proj, np.float64).reshape(4, 4)
    q = pos if prev_pos is None else np.asarray(prev_pos, np.float64).reshape(n, 4)
    # written out, not a matrix product: 0 * inf must give its NaN
    c = np.stack([((m[r, 0] * q[:, 0] + m[r, 1] * q[:, 1]) + m[r, 2] * q[:, 2]) + m[r, 3] for r in range(4)], axis=1)
    u = (c[:, 0] / c[:, 3] + 1.0) / 2.0
    v = (1.0 - c[:, 1] / c[:, 3]) / 2.0
    margin = _no_nan(np.minimum.reduce([np.abs(u), np.abs(u - 1), np.abs(v), np.abs(v - 1)]))
    outside = (u > 1) | (u < 0) | (v > 1) | (v < 0)
    # outside [0,1] of the previous frame: colour kept, spp = 1, nothing accepted, prev_frame_pixel_f not written
    o = proc & outside
    out[o, 3] = 1.0
    S.accept[o] = 0
    ins = proc & ~outside
    pfx, pfy = u * W - 0.5, v * H - 0.5
    ipx, ipy = d3d_int(np.where(ins, pfx, 0), sem), d3d_int(np.where(ins, pfy, 0), sem)
    fx, fy = pfx - ipx, pfy - ipy
    wts = ((1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy)
    mi = _no_nan(np.minimum(_trunc_margin(pfx), _trunc_margin(pfy)))
    accept = np.zeros(n, np.uint32)
    prev = np.zeros((n, 3))
    spp = np.zeros(n)
    tw = np.zeros(n)
    pds, nds = [], []
    for k, (dx, dy) in enumerate(TAPS):
        sx, sy = ipx + dx, ipy + dy
        inb = ins & (sx >= 0) & (sy >= 0) & (sx < W) & (sy < H)
        j = np.where(inb, sy * W + sx, 0)
        pd = np.sum((S.prev_pos[j, :3] - q[:, :3]) ** 2, axis=1)
        nd = np.sum((S.prev_norm[j, :3] - nrm[:, :3]) ** 2, axis=1)
        mi = np.minimum(mi, np.where(inb, _no_nan(np.abs(pd - POSITION_LIMIT_SQUARED) / POSITION_LIMIT_SQUARED), np.inf))
        near = inb & (pd < POSITION_LIMIT_SQUARED)
        mi = np.minimum(mi, np.where(near, _no_nan(np.abs(nd - NORMAL_LIMIT_SQUARED) / NORMAL_LIMIT_SQUARED), np.inf))
        acc = near & (nd < NORMAL_LIMIT_SQUARED)
        accept |= np.where(acc, np.uint32(1 << k), np.uint32(0))
        # a tap that was not accepted adds nothing, whatever its texel holds (0 * NaN would add a NaN)
        spp += np.where(acc, wts[k] * S.prev_noisy[j, 3], 0.0)
        prev += np.where(acc[:, None], wts[k][:, None] * S.prev_noisy[j, :3], 0.0)
        tw += np.where(acc, wts[k], 0.0)
        taps[:, k] = np.where(acc, j, -1)
        pds.append(np.where(inb, pd, np.nan))
        nds.append(np.where(near, nd, np.nan))
    # what the decisions saw, for a test to check which cases a sequence exercised
    S.diag = dict(u=np.where(proc, u, np.nan), v=np.where(proc, v, np.nan), w=c[:, 3], pf=np.stack([pfx, pfy], 1),
                  inside=ins, pd=np.stack(pds, 1), nd=np.stack(nds, 1),
                  # the RG16Float store decides only what postprocess reads
                  half_margin=np.where(ins, np.minimum(_half_margin(pfx), _half_margin(pfy)), np.inf))
    used = tw > 0
    mi = np.minimum(mi, np.where(accept > 0, _no_nan(np.abs(tw)), np.inf))
    tws = np.where(used, tw, 1.0)
    prev /= tws[:, None]
    spp /= tws
    blend = np.where(used, d3d_max(1.0 / (spp + 1.0), BLEND_ALPHA, sem), 1.0)
    new_spp = np.where(blend < 1.0, 1.0 + spp, 1.0)
    res = blend[:, None] * cur + (1.0 - blend[:, None]) * prev
    mi = np.minimum(mi, _inf_blend_margin(blend, cur, prev))
    out[ins, :3] = res[ins]
    out[ins, 3] = new_spp[ins]
    S.accept[ins] = accept[ins]
    pf = np.stack([pfx, pfy], axis=1)
    # out_prev_frame_pixel is RG16Float
    S.prev_pixel[ins] = pf[ins].astype(np.float16).astype(np.float64) if sem.round_prev_pixel else pf[ins]
    margin = np.where(proc, np.minimum(margin, np.where(ins, mi, np.inf)), np.inf)
    taps[~ins] = -1
    return out, margin, taps


def postprocess(S, frame, flags, filtered, sem=D3D):
    """postprocess.ps.hlsl main() for every pixel, reading S's accept bools, prev_frame_pixel_f (float16 values) and
    previous accumulated frame.  Returns (accumulated [n,4], margin [n], taps [n,4])."""
    W, H = S.W, S.H
    n = W * H
    x = np.arange(n) % W
    proc = np.ones(n, bool) if flags & FULL_FRAME else ~((x + 0.5) / W > 0.5)
    acc = filtered.copy()  # texC.x > 0.5: the filtered frame, all four channels
    margin = np.full(n, np.inf)
    taps = np.full((n, 4), -1)
    blend = np.ones(n)
    prev = np.zeros((n, 3))
    if frame > 0:
        live = proc & (S.accept > 0)
        pfx, pfy = S.prev_pixel[:, 0], S.prev_pixel[:, 1]
        ipx, ipy = d3d_int(pfx, sem), d3d_int(pfy, sem)  # int2(): toward zero
        fx, fy = pfx - ipx, pfy - ipy
        wts = ((1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy)
        tw = np.zeros(n)
        for k, (dx, dy) in enumerate(TAPS):
            on = live & ((S.accept & np.uint32(1 << k)) != 0)
            sx, sy = ipx + dx, ipy + dy
            inb = on & (sx >= 0) & (sy >= 0) & (sx < W) & (sy < H)
            j = np.where(inb, sy * W + sx, 0)
            wk = np.where(on, wts[k], 0.0)
            tw += wk
            with np.errstate(all="ignore"):
                prev += wk[:, None] * np.where(inb[:, None], S.prev_filtered[j, :3], 0.0)  # outside the texture: 0
            taps[:, k] = np.where(inb, j, -1)
        margin = np.where(live, _no_nan(np.abs(tw)), np.inf)
        used = live & (tw > 0)
        with np.errstate(all="ignore"):
            blend = np.where(used, d3d_max(1.0 / np.where(used, filtered[:, 3], 1.0), SECOND_BLEND_ALPHA, sem), 1.0)
        prev /= np.where(used, tw, 1.0)[:, None]
        taps[~used] = -1
    with np.errstate(all="ignore"):
        res = blend[:, None] * filtered[:, :3] + (1.0 - blend[:, None]) * prev
        margin = np.minimum(margin, _inf_blend_margin(blend, filtered[:, :3], prev))
    acc[proc, :3] = res[proc]
    acc[proc, 3] = 1.0
    return acc, margin, taps


def execute(S, frame, flags, view_proj, pos, nrm, alb, noisy, amend=None, prev_pos=None, sem=D3D):
    """DenoisePass.cpp:146-204: preprocess, then the three blits to history (noisy, normal, position), then the fit,
    then postprocess, whose result goes both to the output and to BMFR_PrevFiltered.  Returns (out, stages): stages
    maps each stage run to its (result, margin, taps).  amend(noisy) -> noisy, if given, runs after the blits: a test
    may put another implementation's values where this reading's decisions had no margin."""
    pos, nrm, alb, noisy = (np.asarray(a, np.float64).reshape(S.W * S.H, 4) for a in (pos, nrm, alb, noisy))
    stages = {}
    if flags & PREPROCESS:
        noisy, mg, tp = preprocess(S, frame, flags, view_proj, pos, nrm, noisy, prev_pos, sem)
        stages["pre"] = S.last_pre = (noisy, mg, tp)
    S.prev_noisy = noisy.copy()
    S.prev_norm = nrm.copy()
    S.prev_pos = pos.copy()
    if amend is not None:
        noisy = amend(noisy)
    if flags & REGRESSION:
        noisy, mg = fit(S.W, S.H, frame, flags, pos, nrm, alb, S.prev_noisy, sem=sem)
        stages["fit"] = (noisy, mg, None)
    if flags & POSTPROCESS:
        noisy, mg, tp = postprocess(S, frame, flags, noisy, sem)
        stages["post"] = (noisy, mg, tp)
        S.prev_filtered = noisy.copy()
    return noisy, stages
