"""GPU tests of motion (include/bdpt.h "Motion"): the previous pose kept on the device (bdpt_keep_pose), the
PrevWorldPosition channel (bdpt_gbuffer_execute_motion), bdpt_motion_query and the denoiser's motion-aware reprojection
(bdpt_bmfr_execute_motion).  Everything is compared bit for bit: with the plain calls where the contract says they agree,
with the header's interpolation restated in numpy float32, and with bdpt_bmfr_execute fed the previous positions as
features.  Small scenes and frames throughout."""
import ctypes as C
import os

import numpy as np
import pytest

import skin_numpy as sn
from area_scenes import DescArrays, _flags, _light
from test_bmfr import _params, _plane_scene
from test_refit_cpu import deform, positions_of

pytestmark = pytest.mark.gpu

F = np.float32
CHANNELS = ("WorldPosition", "WorldNormal", "MaterialDiffuse", "MaterialSpecRough", "MaterialExtraParams", "Emissive")


def _gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _raw(t):
    """the bytes of a tensor (fp32 or fp16 channel) as a numpy array"""
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy()


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _triangles(desc):
    return np.ctypeslib.as_array(desc.indices, shape=(desc.numTriangles, 3)).astype(np.int64)


def prev_pos_numpy(P, I, prim, u, v):
    """include/bdpt.h "Motion": b0 = 1 - u - v; prev = ((0 + p0*b0) + p1*u) + p2*v per component, float32, one rounding
    per operation.  P (nv, 3) float32 positions of the previous pose, I (nt, 3); prim, u, v per item (all valid prims)."""
    u, v = u.astype(F)[:, None], v.astype(F)[:, None]
    p0, p1, p2 = (P[I[prim, k]].astype(F) for k in range(3))
    b0 = (F(1.0) - u) - v
    pos = np.zeros_like(p0) + p0 * b0
    pos = pos + p1 * u
    pos = pos + p2 * v
    assert pos.dtype == F
    return pos


def _hits(prim, u, v):
    h = np.zeros((len(prim), 4), F)
    h[:, 0], h[:, 1], h[:, 2] = 1.0, u, v
    h.view(np.int32)[:, 3] = prim
    return h


def _corner_hits(nt):
    """every primitive at its three corners, an edge midpoint and an interior point"""
    uv = np.array([[0, 0], [1, 0], [0, 1], [0.5, 0.5], [0.25, 0.375]], F)
    prim = np.repeat(np.arange(nt, dtype=np.int32), len(uv))
    u, v = np.tile(uv[:, 0], nt), np.tile(uv[:, 1], nt)
    return prim, u, v


def _assert_prev_pose(ctx, P, I, label):
    """the context's previous pose holds the corners of positions P: bdpt_motion_query == the restatement"""
    import torch
    prim, u, v = _corner_hits(len(I))
    out = ctx.motion_query(_gpu(_hits(prim, u, v)))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = prev_pos_numpy(P, I, prim, u, v)
    assert np.array_equal(got[:, :3].view(np.uint32), want.view(np.uint32)), f"{label}: {(got[:, :3] != want).any(axis=1).sum()} items differ"
    assert (got[:, 3] == 1.0).all(), label


# ---- 1. an unmoved scene: the channel is WorldPosition, everything else is bdpt_gbuffer_execute ----

def test_unmoved_scene_channel_equals_world_position(pkg):
    """The foliage courtyard (textured, alpha-masked) at 44x28, pinhole and thin lens: after prepare(motion) and again after
    keep_pose without an update, prevPosition equals worldPosition in every pixel as raw words (w included); the six channels
    and the next bdpt_execute frame equal those of a context that ran bdpt_gbuffer_execute."""
    import torch
    scene = pkg.Scene.courtyard(1, 20000)
    W, H = 44, 28
    plain = pkg.FramePipeline(scene, W, H, max_depth=3)
    mot = pkg.FramePipeline(scene, W, H, max_depth=3, motion=True)
    assert mot.prev_position is not None and plain.prev_position is None
    st = mot._stream_ptr()
    for step, (thin, keep) in enumerate([(False, False), (True, False), (False, True), (True, True)]):
        if keep:
            mot.ctx.keep_pose(st)
        for pipe in (plain, mot):
            pipe.gbuffer_frame, pipe.bdpt_frame = 0xdeadbeef + step, 0x1337 + step
        gp = plain.gbuffer_params()
        gp.useThinLens = 1 if thin else 0
        mot.prev_position.fill_(7.0)
        plain.ctx.gbuffer_execute(gp, plain.gb, st)
        mot.ctx.gbuffer_execute_motion(gp, mot.gb, _ptr(mot.prev_position), st)
        p = plain.bdpt_params()
        plain.ctx.execute(p, plain.gb, _ptr(plain.output), st)
        mot.ctx.execute(p, mot.gb, _ptr(mot.output), st)
        torch.cuda.synchronize()
        for name in CHANNELS:
            assert np.array_equal(_raw(plain.channels[name]), _raw(mot.channels[name])), (name, thin, keep)
        pos, prev = _raw(mot.channels["WorldPosition"]), _raw(mot.prev_position)
        assert np.array_equal(pos, prev), (thin, keep)
        w = mot.prev_position[..., 3].cpu().numpy()
        assert (w == 1).sum() > W * H // 2 and ((w == 0) | (w == 1)).all()
        assert np.array_equal(_raw(plain.output), _raw(mot.output)), (thin, keep)
    plain.close()
    mot.close()
    scene.close()


# ---- 2. the interpolation against numpy float32 ----

def test_motion_query_equals_the_restatement_after_an_update(pkg):
    """A soup of 5 000 triangles moved by an update: bdpt_motion_query on random hits (u + v = 1 edges, u = v = 0, misses,
    prims outside the scene) equals the header's expression on the PRE-update corners; items at or beyond *numDevice stay
    untouched; host arrays go the copied path."""
    import torch
    scene = pkg.Scene.soup(11, 5000, 0.1)
    d = scene.desc
    nt = int(d.numTriangles)
    P0, I = positions_of(d), _triangles(d)
    P1 = deform(P0)
    ctx = pkg.Context(0)
    ctx.set_scene(d)
    ctx.prepare(motion=True)
    ctx.keep_pose()
    ctx.update_geometry(P1)
    rng = np.random.default_rng(5)
    n = 4099  # (no multiple of 64)
    prim = rng.integers(0, nt, n).astype(np.int32)
    u = rng.uniform(0, 1, n).astype(F)
    v = (rng.uniform(0, 1, n).astype(F) * (F(1) - u)).astype(F)
    v[:300] = F(1) - u[:300]     # on the edge opposite corner 0
    u[300:400] = v[300:400] = 0  # corner 0
    u[400:450], v[400:450] = 1, 0
    bad = np.zeros(n, bool)
    prim[500:560], bad[500:560] = -1, True
    prim[560:570], bad[560:570] = nt, True
    prim[570:575], bad[570:575] = 2**31 - 1, True
    prim[575:580], bad[575:580] = -2**31, True
    hits = _hits(prim, u, v)
    th = _gpu(hits)
    out = ctx.motion_query(th)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = np.zeros((n, 4), F)
    want[~bad, :3] = prev_pos_numpy(P0, I, prim[~bad], u[~bad], v[~bad])
    want[~bad, 3] = 1.0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{(got != want).any(axis=1).sum()} items differ"
    moved = prev_pos_numpy(P1, I, prim[~bad], u[~bad], v[~bad])
    assert (moved != want[~bad, :3]).any(axis=1).mean() > 0.9  # (the update did move the corners)
    # a device count: the items at or beyond it are untouched, also in the last, ragged wave
    for cnt in (0, 1, 64, 1000, n, n + 7):
        res = torch.full((n, 4), 7.0, dtype=torch.float32, device="cuda")
        count = torch.tensor([cnt], dtype=torch.int32, device="cuda")
        ctx.motion_query(th, out=res, count=count)
        torch.cuda.synchronize()
        r = res.cpu().numpy()
        k = min(cnt, n)
        assert np.array_equal(r[:k].view(np.uint32), want[:k].view(np.uint32)) and (r[k:] == 7.0).all(), cnt
    host = ctx.motion_query(hits)
    assert isinstance(host, np.ndarray) and np.array_equal(host.view(np.uint32), want.view(np.uint32))
    ctx.close()
    scene.close()


def test_gbuffer_channel_equals_camera_rays_trace_motion_query(pkg):
    """The moved Cornell box at 48x32: the PrevWorldPosition channel equals camera_rays -> trace_rays (closest hit, back
    faces culled: the G-buffer's query) -> motion_query of the same frame, and differs from WorldPosition where the
    surface moved."""
    import torch
    scene = pkg.Scene.cornell()
    W, H = 48, 32
    pipe = pkg.FramePipeline(scene, W, H, max_depth=3, motion=True)
    st = pipe._stream_ptr()
    P0 = positions_of(scene.desc)
    pipe.ctx.keep_pose(st)
    pipe.update_geometry(deform(P0, seed=5, amp=0.01))
    for thin in (False, True):
        gp = pipe.gbuffer_params()
        gp.useThinLens = 1 if thin else 0
        rays = pipe.ctx.camera_rays(gp, W, H, stream=st)
        hits = torch.empty((W * H, 4), dtype=torch.float32, device="cuda")
        pipe.ctx.trace_rays(rays, "closest_cull_back", out=hits, stream=st)
        q = pipe.ctx.motion_query(hits, stream=st)
        pipe.ctx.gbuffer_execute_motion(gp, pipe.gb, _ptr(pipe.prev_position), st)
        torch.cuda.synchronize()
        assert np.array_equal(_raw(q), _raw(pipe.prev_position.reshape(-1, 4))), thin
        pos, prev = pipe.channels["WorldPosition"].cpu().numpy(), pipe.prev_position.cpu().numpy()
        assert np.array_equal(pos[..., 3], prev[..., 3])
        hit = pos[..., 3] == 1
        assert hit.sum() > W * H // 2 and (pos[hit][:, :3] != prev[hit][:, :3]).any(axis=1).mean() > 0.5
    pipe.close()
    scene.close()


# ---- 3. pose bookkeeping ----

@pytest.mark.parametrize("num_triangles", [1, 63, 64, 65, 130])
def test_pose_bookkeeping(pkg, num_triangles):
    """keep_pose; update A; keep_pose; update B -> the previous pose is A.  Two updates without a keep_pose between them
    leave it alone.  keep_pose twice without an update: previous == current.  The same through update_skinned.  Primitive
    counts around one wave of the copy kernel (its last wave ragged, full, one lane, two waves and a bit)."""
    scene = pkg.Scene.soup(20 + num_triangles, num_triangles, 0.3)
    d = scene.desc
    assert int(d.numTriangles) == num_triangles
    P0, I = positions_of(d), _triangles(d)
    A, B = deform(P0, seed=3), deform(P0, seed=4)
    ctx = pkg.Context(0)
    ctx.set_scene(d)
    ctx.prepare(motion=True)
    _assert_prev_pose(ctx, P0, I, "after prepare: previous == current")
    ctx.keep_pose()
    _assert_prev_pose(ctx, P0, I, "keep_pose without an update")
    ctx.update_geometry(A)
    _assert_prev_pose(ctx, P0, I, "an update alone does not touch the previous pose")
    ctx.keep_pose()
    ctx.update_geometry(B)
    _assert_prev_pose(ctx, A, I, "keep; update A; keep; update B")
    ctx.update_geometry(P0)
    ctx.update_geometry(B)
    _assert_prev_pose(ctx, A, I, "two updates without a keep_pose")
    ctx.keep_pose()
    ctx.keep_pose()
    _assert_prev_pose(ctx, B, I, "keep_pose twice: previous == current")
    # skinning: positions only (a soup has no use for its normals here)
    nb = 5
    r = sn.scene_rig(d, 7, nb)
    ctx.set_skin(r["P"], r["W"], r["I"], nb)
    poses = [sn.make_pose(s, nb, r["pivot"], r["extent"]) for s in (1, 2)]
    S = [sn.skin(r["P"], r["W"], r["I"], bones)[0] for bones, _ in poses]
    ctx.keep_pose()
    ctx.update_skinned(poses[0][0])
    _assert_prev_pose(ctx, B, I, "skinned: an update alone")
    ctx.keep_pose()
    ctx.update_skinned(poses[1][0])
    _assert_prev_pose(ctx, S[0], I, "skinned: keep; pose 1; keep; pose 2")
    ctx.keep_pose()
    _assert_prev_pose(ctx, S[1], I, "skinned: keep_pose after the last update")
    ctx.close()
    scene.close()


# ---- 4. / 5. the denoiser: composition with, and degenerate equality to, bdpt_bmfr_execute ----

class _Bmfr:
    """A context sized with resize (no scene) fed synthetic G-buffers, as test_bmfr._SyntheticBmfr"""

    def __init__(self, pkg, W, H):
        import torch
        self.torch, self.pkg, self.W, self.H = torch, pkg, W, H
        self.lib = pkg.load_library()
        self.ctx = pkg.Context(0)
        self.ctx.resize(W, H, 0, H, 1)

    def run(self, p, pos, nrm, alb, noisy, prev=None, alias=False):
        torch = self.torch
        t_pos, t_noisy = _gpu(pos), _gpu(noisy)
        t_nrm, t_alb = _gpu(nrm.astype(np.float16)), _gpu(alb.astype(np.float16))
        gb = self.pkg.abi.GBuffer()
        gb.worldPosition, gb.worldNormal, gb.materialDiffuse = t_pos.data_ptr(), t_nrm.data_ptr(), t_alb.data_ptr()
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if alias:
            self.ctx.bmfr_execute_motion(p, gb, _ptr(t_pos), _ptr(t_noisy), st)
        elif prev is not None:
            t_prev = _gpu(prev)
            self.ctx.bmfr_execute_motion(p, gb, _ptr(t_prev), _ptr(t_noisy), st)
        else:
            self.ctx.bmfr_execute(p, gb, _ptr(t_noisy), st)
        torch.cuda.synchronize()
        return t_noisy.cpu().numpy()

    def history(self):
        n = C.c_uint64()
        assert self.lib.bdpt_bmfr_history_bytes(self.ctx._h, C.byref(n)) == 0 and n.value == self.W * self.H * 64
        blob = np.zeros(n.value // 4, F)
        assert self.lib.bdpt_bmfr_save_history(self.ctx._h, blob.ctypes.data, n.value) == 0
        return blob.reshape(4, self.H * self.W, 4)  # position, normal, noisy, filtered

    def load(self, blob):
        blob = np.ascontiguousarray(blob, F)
        assert self.lib.bdpt_bmfr_load_history(self.ctx._h, blob.ctypes.data, blob.nbytes) == 0

    def close(self):
        self.ctx.close()


def test_bmfr_motion_is_bmfr_with_the_previous_positions_as_features(pkg):
    """40x24 synthetic features, a loaded history.  bdpt_bmfr_execute_motion with features position P and prevPosition Q
    against bdpt_bmfr_execute with features position Q, flags PREPROCESS and PREPROCESS | POSTPROCESS: the noisy outputs
    are bit-identical, and the saved histories differ only in the position plane, which holds P for the motion call."""
    A = pkg.abi
    W, H = 40, 24
    rng = np.random.default_rng(12)
    P, nrm, alb, noisy, _ = _plane_scene(W, H, rng)
    # Q: the upper rows moved three pixels' worth along x, a band moved 0.5 in depth (the projection ignores z here: the same
    # taps, none of which passes the position test), the rest unmoved
    Q = P.copy().reshape(H, W, 4)
    Q[:10, :, 0] -= F(0.06)
    Q[10:14, :, 2] += F(0.5)
    Q = Q.reshape(-1, 4)
    vp = np.zeros((4, 4), F)
    vp[0, 0], vp[1, 1], vp[3, 3] = 1.0 / (0.02 * W / 2), 1.0 / (0.02 * H / 2), 1.0
    hist = np.zeros((4, H * W, 4), F)
    hist[0], hist[1] = P, nrm
    hist[2, :, :3] = rng.uniform(0, 1, (H * W, 3))
    hist[2, :, 3] = rng.integers(1, 6, H * W)  # spp of the history
    hist[3] = rng.uniform(0, 1, (H * W, 4))
    mot, ref = _Bmfr(pkg, W, H), _Bmfr(pkg, W, H)
    for flags in (A.BMFR_PREPROCESS, A.BMFR_PREPROCESS | A.BMFR_POSTPROCESS, A.BMFR_PREPROCESS | A.BMFR_FULL_FRAME,
                  A.BMFR_PREPROCESS | A.BMFR_POSTPROCESS | A.BMFR_FULL_FRAME):
        p = _params(pkg, 1, flags, list(vp.reshape(-1)))
        mot.load(hist)
        ref.load(hist)
        a = mot.run(p, P, nrm, alb, noisy.copy(), prev=Q)
        b = ref.run(p, Q, nrm, alb, noisy.copy())
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"flags {flags}: {(a != b).any(axis=1).sum()} pixels differ"
        assert not np.array_equal(a, noisy)
        if flags == A.BMFR_PREPROCESS | A.BMFR_FULL_FRAME:  # the moved rows found history three pixels to the left: spp = 1 + its spp
            spp = a.reshape(H, W, 4)[2:8, 8:-8, 3]
            assert (spp >= 2).all() and (a.reshape(H, W, 4)[10:14, :, 3] == 1).all()
        ha, hb = mot.history(), ref.history()
        assert np.array_equal(ha[0].view(np.uint32), P.view(np.uint32)), "the history stores the CURRENT position"
        assert np.array_equal(hb[0].view(np.uint32), Q.view(np.uint32))
        assert np.array_equal(ha[1:].view(np.uint32), hb[1:].view(np.uint32)), flags
    mot.close()
    ref.close()


@pytest.mark.parametrize("full", [False, True], ids=["half", "full"])
def test_bmfr_motion_with_unmoved_positions_is_bmfr(pkg, full):
    """prevPosition aliasing (or equal to) worldPosition: four frames of the moving synthetic sequence with every stage on
    (regression included) equal bdpt_bmfr_execute bit for bit, outputs and the history blob."""
    import test_bmfr_cross_check as xc
    A = pkg.abi
    W, H = 40, 24
    flags = A.BMFR_PREPROCESS | A.BMFR_REGRESSION | A.BMFR_POSTPROCESS | (A.BMFR_FULL_FRAME if full else 0)
    ref, alias, equal = _Bmfr(pkg, W, H), _Bmfr(pkg, W, H), _Bmfr(pkg, W, H)
    for k in range(4):
        (pos, nrm, alb, noisy), vp = xc.sequence_gbuffer(pkg, W, H, k)
        p = _params(pkg, k, flags, vp)
        want = ref.run(p, pos, nrm, alb, noisy.copy())
        a = alias.run(p, pos, nrm, alb, noisy.copy(), alias=True)
        e = equal.run(p, pos, nrm, alb, noisy.copy(), prev=pos.copy())
        for got, label in ((a, "aliasing"), (e, "equal")):
            same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
            assert same.all(), f"frame {k}, {label}: {(~same).any(axis=1).sum()} pixels differ"
    hr = ref.history().view(np.uint32)
    assert np.array_equal(alias.history().view(np.uint32), hr) and np.array_equal(equal.history().view(np.uint32), hr)
    for b in (ref, alias, equal):
        b.close()


# ---- 6. what it is for: a moving surface keeps its history ----

class _SlidingScene(DescArrays):
    """A wall (z = 0) and, in front of it, a large triangle tilted about the vertical axis that slides along x; the camera
    looks down -z from (0, 0, 10).  Both double-sided, one material.  Every coordinate is a multiple of 1/16, so that a
    whole-unit shift is exact in float32."""
    CAM = ((0.0, 0.0, 10.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    FOCAL, FRAME_H = 30.0, 24.0  # tan(fovY / 2) = 0.4: at the triangle (4 units away) a 32-row frame's pixel is 0.1 units
    TRI = 2                      # primitive index of the moving triangle

    def __init__(self, pkg):
        a = pkg.abi
        m = a.Material()
        m.baseColor[:] = (0.6, 0.6, 0.6, 1.0)
        m.specular[:] = (0.0, 1.0, 0.0, 0.0)
        m.alphaThreshold, m.IoR = 0.5, 1.5
        m.texBaseColor = m.texSpecular = m.texEmissive = m.texNormal = -1
        m.flags = _flags(1, 1, 0) | (1 << 19)  # double-sided
        wall = np.array([[-8, -6, 0], [8, -6, 0], [8, 6, 0], [-8, 6, 0]], F)
        # z = 6 + (x + 1.5) / 4 at offset 0: 1 unit along x changes the depth under a fixed pixel by about 0.25
        tri = np.array([[-2.25, -1.0, 5.8125], [-0.75, -1.0, 6.1875], [-1.5, 1.25, 6.0]], F)
        P = np.concatenate([wall, tri])
        n_tri = np.cross(tri[1] - tri[0], tri[2] - tri[0])
        n_tri = (n_tri / np.linalg.norm(n_tri)).astype(F)
        N = np.concatenate([np.tile([[0, 0, 1]], (4, 1)).astype(F), np.tile(n_tri, (3, 1))])
        I = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6]], np.uint32)
        super().__init__(a, P, N, np.zeros((7, 3), F), I, np.zeros(3, np.uint32), [m], [],
                         [_light(a, a.LIGHT_POINT, (0.0, 5.0, 9.0), (0.0, -1.0, 0.0), (10.0, 10.0, 10.0))])
        self.pkg = pkg

    def at(self, offset):
        P = self.P.copy()
        P[4:, 0] += F(offset)
        return P

    def camera(self, aspect):
        cam = self.pkg.abi.Camera()
        v3 = lambda v: (C.c_float * 3)(*v)
        pos, tgt, up = self.CAM
        assert self.pkg.load_library().bdpt_camera_look_at(v3(pos), v3(tgt), v3(up), self.FOCAL, self.FRAME_H, aspect, 1.0, C.byref(cam)) == 0
        return cam

    def view_proj(self, aspect):
        pos, tgt, up = self.CAM
        return self.pkg.camera_view_proj(pos, tgt, up, self.FOCAL, self.FRAME_H, aspect, 0.1, 1000.0)


def _footprint(q, m, W, H):
    """bmfr_preprocess_kernel's reprojection of positions q (N, 3) restated in float32: (inside the frame, ipx, ipy) —
    the history taps are (ipx + 0|1, ipy + 0|1)"""
    m = np.asarray(m, F)
    c = [((m[4 * r] * q[:, 0] + m[4 * r + 1] * q[:, 1]) + m[4 * r + 2] * q[:, 2]) + m[4 * r + 3] for r in range(4)]
    ux, uy = c[0] / c[3], c[1] / c[3]
    ux, uy = (ux + F(1)) / F(2), (F(1) - uy) / F(2)
    inside = ~((ux > 1) | (ux < 0) | (uy > 1) | (uy < 0))
    pfx, pfy = ux * F(W) - F(0.5), uy * F(H) - F(0.5)
    assert pfx.dtype == F
    return inside, pfx.astype(np.int32), pfy.astype(np.int32)


def _footprint_all(mask_prev, inside, ipx, ipy, W, H):
    """per pixel: all four taps lie in the frame and on pixels of mask_prev (H, W)"""
    ok = inside & (ipx >= 0) & (ipy >= 0) & (ipx + 1 < W) & (ipy + 1 < H)
    x, y = np.clip(ipx, 0, W - 2), np.clip(ipy, 0, H - 2)
    for dy in (0, 1):
        for dx in (0, 1):
            ok &= mask_prev[y + dy, x + dx]
    return ok


def test_moving_surface_keeps_its_history(pkg):
    """A triangle slides 1.0 world unit per frame in front of a static wall, static camera, 48x32, three frames of
    keep_pose -> update_geometry -> gbuffer_execute_motion -> bmfr (PREPROCESS) on constant-plus-noise input.

    Selected pixels of a frame (from the trace_rays prim ids of consecutive frames): those on the triangle whose whole 2x2
    reprojected footprint lay on the triangle in the previous frame — for the third frame also that the footprint's pixels
    were selected in the second: a tap that had no history itself carries spp 1 into the average by the unchanged blend
    rules, whichever call made it.  With the motion call their spp (noisy.w) is 2, then 3; with bdpt_bmfr_execute on
    identical inputs it stays 1, because the world position under a fixed pixel changed by more than the 0.1-unit threshold.
    On wall pixels whose footprint is wall in both frames the two calls agree bit for bit."""
    import torch
    A = pkg.abi
    W, H = 48, 32
    scene = _SlidingScene(pkg)
    TRI = scene.TRI
    vp = scene.view_proj(W / H)
    pipes = {name: pkg.FramePipeline(scene, W, H, max_depth=2, mat_index=1, motion=True) for name in ("motion", "plain")}
    rng = np.random.default_rng(3)
    spp, outs, prims, sel = {n: [] for n in pipes}, {n: [] for n in pipes}, [], []
    wall_sel, tri_any = [], np.zeros((H, W), bool)
    for k in range(3):
        noisy = np.ones((H, W, 4), F)
        noisy[..., :3] = 0.5 + 0.1 * rng.standard_normal((H, W, 3)).astype(F)
        for name, pipe in pipes.items():
            st = pipe._stream_ptr()
            pipe.use_jitter = False
            pipe.ctx.keep_pose(st)
            pipe.update_geometry(scene.at(k))
            gp = pipe.gbuffer_params()
            pipe.ctx.gbuffer_execute_motion(gp, pipe.gb, _ptr(pipe.prev_position), st)
            t = _gpu(noisy)
            p = _params(pkg, k, A.BMFR_PREPROCESS | A.BMFR_FULL_FRAME, vp)
            if name == "motion":
                pipe.ctx.bmfr_execute_motion(p, pipe.gb, _ptr(pipe.prev_position), _ptr(t), st)
            else:
                pipe.ctx.bmfr_execute(p, pipe.gb, _ptr(t), st)
            torch.cuda.synchronize()
            o = t.cpu().numpy()
            outs[name].append(o)
            spp[name].append(o[..., 3])
        pipe = pipes["motion"]
        rays = pipe.ctx.camera_rays(gp, W, H)
        hits = torch.empty((W * H, 4), dtype=torch.float32, device="cuda")
        pipe.ctx.trace_rays(rays, "closest_cull_back", out=hits)
        torch.cuda.synchronize()
        prim = hits.cpu().numpy().view(np.int32)[:, 3].reshape(H, W)
        prims.append(prim)
        tri_any |= prim == TRI
        assert (prim == TRI).sum() > 100 and (prim >= 0).all(), "the triangle is in view and the wall fills the frame"
        if k == 0:
            assert all((s[0] == 1).all() for s in spp.values())
            sel.append(None)
            continue
        q = pipe.prev_position.cpu().numpy().reshape(-1, 4)[:, :3]
        inside, ipx, ipy = _footprint(q, vp, W, H)
        on_tri = _footprint_all(prims[k - 1] == TRI, inside, ipx, ipy, W, H).reshape(H, W) & (prim == TRI)
        if k == 2:
            on_tri &= _footprint_all(sel[1], inside, ipx, ipy, W, H).reshape(H, W)
        sel.append(on_tri)
        on_wall = _footprint_all(prims[k - 1] != TRI, inside, ipx, ipy, W, H).reshape(H, W) & (prim != TRI)
        wall_sel.append((on_wall, (inside, ipx, ipy)))
        print(f"frame {k}: {on_tri.sum()} selected triangle pixels, {on_wall.sum()} wall pixels; motion spp there "
              f"{np.unique(spp['motion'][k][on_tri])}, plain spp there {np.unique(spp['plain'][k][on_tri])}, "
              f"wall spp {np.unique(spp['motion'][k][on_wall])}", flush=True)
    for k in (1, 2):
        assert sel[k].sum() >= 20, (k, sel[k].sum())
        assert (spp["motion"][k][sel[k]] == k + 1).all(), (k, np.unique(spp["motion"][k][sel[k]]))
        assert (spp["plain"][k][sel[k]] == 1).all(), (k, np.unique(spp["plain"][k][sel[k]]))
        ws, fp = wall_sel[k - 1]
        assert ws.sum() > 200
        assert np.array_equal(outs["motion"][k][ws].view(np.uint32), outs["plain"][k][ws].view(np.uint32)), k
        # (where the triangle never was, the static wall converges under both calls: the reprojection finds its own pixel)
        static = ws & _footprint_all(~tri_any, *fp, W, H).reshape(H, W)
        assert static.sum() > 200 and (spp["motion"][k][static] == k + 1).all(), np.unique(spp["motion"][k][static])
    for pipe in pipes.values():
        pipe.close()


# ---- 7. capture ----

def test_keep_pose_update_and_motion_gbuffer_captured_in_a_hip_graph(pkg):
    """keep_pose -> update_skinned (device bones) -> gbuffer_execute_motion captured in one hipGraph and replayed with two
    palettes (A, B, A): the six channels and PrevWorldPosition of every replay equal the eager calls'.  The replayed
    keep_pose runs every time: the third replay's previous pose is B's."""
    import torch
    scene = pkg.Scene.cornell()
    d = scene.desc
    W, H, nb = 48, 32, 4
    r = sn.scene_rig(d, 31, nb)
    poses = [sn.make_pose(s, nb, r["pivot"], r["extent"], angle=0.04, shift=0.005) for s in (41, 42, 43)]
    pipe = pkg.FramePipeline(scene, W, H, max_depth=3, motion=True)
    pipe.set_skin(r["P"], r["W"], r["I"], nb, r["N"], r["B"])
    tb, tn = _gpu(poses[0][0]), _gpu(poses[0][1])
    gp = pipe.gbuffer_params()
    side = torch.cuda.Stream()
    order = (0, 1, 0)

    def load(k):
        tb.copy_(torch.from_numpy(poses[k][0]))
        tn.copy_(torch.from_numpy(poses[k][1]))
        torch.cuda.synchronize()

    def start():  # previous == current == the third pose
        load(2)
        with torch.cuda.stream(side):
            pipe.update_skinned(tb, tn)
            pipe.ctx.keep_pose(pipe._stream_ptr())
        torch.cuda.synchronize()

    def sequence():
        st = pipe._stream_ptr()
        pipe.ctx.keep_pose(st)
        pipe.update_skinned(tb, tn)
        pipe.ctx.gbuffer_execute_motion(gp, pipe.gb, _ptr(pipe.prev_position), st)

    def snapshot():
        return [_raw(pipe.channels[n]).copy() for n in CHANNELS] + [_raw(pipe.prev_position).copy()]

    start()
    refs = []
    for k in order:
        load(k)
        with torch.cuda.stream(side):
            sequence()
        torch.cuda.synchronize()
        refs.append(snapshot())
    assert not np.array_equal(refs[0][-1], refs[2][-1]) and np.array_equal(refs[0][0], refs[2][0])  # same pose, another previous one
    assert not np.array_equal(refs[0][0], refs[0][-1])
    start()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        sequence()
        graph.capture_end()
    torch.cuda.synchronize()
    for i, k in enumerate(order):
        load(k)
        for n in CHANNELS:
            pipe.channels[n].zero_()
        pipe.prev_position.fill_(7.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for got, want, name in zip(snapshot(), refs[i], CHANNELS + ("PrevWorldPosition",)):
            assert np.array_equal(got, want), (i, name)
    del graph
    pipe.close()
    scene.close()


# ---- 8. errors ----

def test_motion_error_conventions(pkg):
    """Every code of include/bdpt.h "Motion"; a refused call enqueues nothing and leaves the scene usable: the frame after
    them equals the frame before.  bdpt_set_scene drops the previous pose; bdpt_prepare(BDPT_PREPARE_MOTION) is refused
    inside a stream capture without breaking it."""
    import torch
    lib, a = pkg.load_library(), pkg.abi
    scene = pkg.Scene.cornell()
    W, H = 32, 24
    buf = torch.zeros(W * H + 1, 4, dtype=torch.float32, device="cuda")
    hits = torch.zeros(64, 4, dtype=torch.float32, device="cuda")
    out = torch.full((65, 4), 7.0, dtype=torch.float32, device="cuda")
    gp, bp = a.GBufferParams(), _params(pkg, 0, a.BMFR_PREPROCESS)

    def desc(h=hits.data_ptr(), n=64, reserved=0, count=None, o=out.data_ptr()):
        d = a.MotionDesc()
        d.hits, d.num, d.reserved, d.numDevice, d.prevPositions = h, n, reserved, count, o
        return d

    # no scene
    ctx = pkg.Context(0)
    gb0 = a.GBuffer()
    assert lib.bdpt_prepare(ctx._h, a.PREPARE_MOTION) == -2
    assert lib.bdpt_keep_pose(ctx._h, None) == -2
    assert lib.bdpt_motion_query(ctx._h, C.byref(desc()), None) == -2
    assert lib.bdpt_gbuffer_execute_motion(ctx._h, C.byref(gp), C.byref(gb0), buf.data_ptr(), None) == -2
    ctx.close()
    # a scene, a camera and a size, but no previous pose
    pipe = pkg.FramePipeline(scene, W, H, max_depth=2)
    h, st = pipe.ctx._h, pipe._stream_ptr()
    gp = pipe.gbuffer_params()
    assert lib.bdpt_keep_pose(h, st) == -2
    assert lib.bdpt_motion_query(h, C.byref(desc()), st) == -2
    assert lib.bdpt_motion_query(h, C.byref(desc(n=0)), st) == -2
    assert lib.bdpt_gbuffer_execute_motion(h, C.byref(gp), C.byref(pipe.gb), buf.data_ptr(), st) == -2
    # ... and BDPT_PREPARE_MOTION inside a capture (the context's last call is in it)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        pipe.ctx.gbuffer_execute(gp, pipe.gb, pipe._stream_ptr())
        assert lib.bdpt_prepare(h, a.PREPARE_MOTION) == -2
        graph.capture_end()
    torch.cuda.synchronize()
    del graph
    assert lib.bdpt_keep_pose(h, st) == -2  # (nothing was prepared)
    pipe.ctx.prepare(motion=True)
    pipe.ctx.prepare(motion=True)  # (again: nothing to do)
    pipe.ctx.gbuffer_execute_motion(gp, pipe.gb, C.c_void_p(buf.data_ptr()), st)
    torch.cuda.synchronize()
    before = [_raw(pipe.channels[n]).copy() for n in CHANNELS] + [_raw(buf).copy()]
    # refused arguments
    assert lib.bdpt_gbuffer_execute_motion(h, C.byref(gp), C.byref(pipe.gb), None, st) == -1
    assert lib.bdpt_gbuffer_execute_motion(h, C.byref(gp), C.byref(pipe.gb), buf.data_ptr() + 4, st) == -1
    assert lib.bdpt_gbuffer_execute_motion(h, None, C.byref(pipe.gb), buf.data_ptr(), st) == -1
    assert lib.bdpt_gbuffer_execute_motion(h, C.byref(gp), None, buf.data_ptr(), st) == -1
    assert lib.bdpt_gbuffer_execute_motion(h, C.byref(gp), C.byref(gb0), buf.data_ptr(), st) == -1  # channels missing
    assert lib.bdpt_motion_query(h, None, st) == -1
    for d, label in ((desc(h=None), "hits"), (desc(o=None), "prevPositions"), (desc(h=hits.data_ptr() + 4), "hits alignment"),
                     (desc(o=out.data_ptr() + 8), "prevPositions alignment"), (desc(count=out.data_ptr() + 2), "numDevice alignment"),
                     (desc(reserved=1), "reserved")):
        assert lib.bdpt_motion_query(h, C.byref(d), st) == -1, label
    assert lib.bdpt_motion_query(h, C.byref(desc(h=None, n=0, o=None)), st) == 0  # num == 0: nothing to do
    noisy = torch.ones(H, W, 4, dtype=torch.float32, device="cuda")
    assert lib.bdpt_bmfr_execute_motion(h, C.byref(bp), C.byref(pipe.gb), None, noisy.data_ptr(), st) == -1
    assert lib.bdpt_bmfr_execute_motion(h, C.byref(bp), C.byref(pipe.gb), buf.data_ptr() + 4, noisy.data_ptr(), st) == -1
    assert lib.bdpt_bmfr_execute_motion(h, C.byref(bp), C.byref(pipe.gb), buf.data_ptr(), None, st) == -1
    assert lib.bdpt_bmfr_execute_motion(h, None, C.byref(pipe.gb), buf.data_ptr(), noisy.data_ptr(), st) == -1
    assert lib.bdpt_bmfr_execute_motion(h, C.byref(bp), C.byref(gb0), buf.data_ptr(), noisy.data_ptr(), st) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (noisy == 1.0).all()  # nothing was enqueued
    pipe.ctx.keep_pose(st)
    pipe.ctx.gbuffer_execute_motion(gp, pipe.gb, C.c_void_p(buf.data_ptr()), st)
    torch.cuda.synchronize()
    after = [_raw(pipe.channels[n]) for n in CHANNELS] + [_raw(buf)]
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    # a new scene drops the previous pose
    pipe.ctx.set_scene(scene.desc)
    assert lib.bdpt_keep_pose(h, st) == -2
    assert lib.bdpt_motion_query(h, C.byref(desc()), st) == -2
    pipe.ctx.set_camera(pipe.cam)
    assert lib.bdpt_gbuffer_execute_motion(h, C.byref(gp), C.byref(pipe.gb), buf.data_ptr(), st) == -2
    pipe.ctx.prepare(motion=True)
    pipe.ctx.gbuffer_execute_motion(gp, pipe.gb, C.c_void_p(buf.data_ptr()), st)
    torch.cuda.synchronize()
    assert all(np.array_equal(x, y) for x, y in zip(before, [_raw(pipe.channels[n]) for n in CHANNELS] + [_raw(buf)]))
    pipe.close()
    scene.close()


# ---- 9. the C++ host ----

def _bend_rig(P):
    """host/main.cpp's --bend rig restated in float32: four bones stacked along the scene's height, every vertex blended
    between the two next to it; (weights, ids, pivot)"""
    kb = 4
    lo, hi = P.min(axis=0), P.max(axis=0)
    pivot = np.array([F(0.5) * (lo[0] + hi[0]), lo[1], F(0.5) * (lo[2] + hi[2])], F)
    height = max(hi[1] - lo[1], F(1e-20))
    s = np.minimum(np.maximum((P[:, 1] - lo[1]) / height, F(0)), F(1)) * F(kb - 1)
    k = np.minimum(s.astype(np.uint32), kb - 2)
    f = s - k.astype(F)
    W = np.zeros((len(P), 4), F)
    ids = np.zeros((len(P), 4), np.uint16)
    ids[:, 0], ids[:, 1] = k, k + 1
    W[:, 0], W[:, 1] = F(1) - f, f
    return W, ids, pivot


def _bend_bones(libm, bend, frame, pivot):
    """the palette main.cpp builds before frame `frame`, with the C library's own sinf / cosf"""
    kb = 4
    bones, nbones = np.zeros((kb, 16), F), np.zeros((kb, 16), F)
    for k in range(kb):
        a = F(F(F(bend) * F(libm.sinf(float(F(0.7) * F(frame + 1))))) * F(k)) / F(kb - 1)
        cs, s = F(libm.cosf(float(a))), F(libm.sinf(float(a)))
        R = np.array([cs, s, 0, -s, cs, 0, 0, 0, 1], F)
        for r in range(3):
            bones[k, 4 * r:4 * r + 3] = nbones[k, 4 * r:4 * r + 3] = R[3 * r:3 * r + 3]
        for c in range(3):
            bones[k, 12 + c] = pivot[c] - ((pivot[0] * R[c] + pivot[1] * R[3 + c]) + pivot[2] * R[6 + c])
        bones[k, 15] = nbones[k, 15] = 1.0
    return bones, nbones


def test_cpp_host_bend_denoise_matches_python_sequence(pkg, tmp_path):
    """host/bdpt_render --bend --denoise (the denoiser asks for PrevWorldPosition, the G-buffer pass renders it, the
    pipeline keeps the pose once per frame) == the same calls driven from Python; with --no-motion it equals the plain
    calls (what the program gave before there was motion), and the program says which of the two it ran.  The two images
    themselves coincide here: a pixel of this 48x32 frame spans about 17 units of the Cornell box, so no history tap lies
    within the denoiser's 0.1 units of a moved point whichever way it is reprojected (test_moving_surface_keeps_its_history
    is where the two calls differ)."""
    import subprocess
    import torch
    import __graft_entry__ as ge
    A = pkg.abi
    exe = os.path.join(ge.PKG_DIR, "host", "bdpt_render")
    assert os.path.exists(exe), "host/bdpt_render not built (run __graft_entry__.build())"
    W, H, frames, bend = 48, 32, 3, 0.3
    cpp = {}
    for name, extra in (("motion", []), ("plain", ["--no-motion"])):
        raw = tmp_path / f"{name}.f32"
        r = subprocess.run([exe, "--scene", "cornell", "--width", str(W), "--height", str(H), "--frames", str(frames), "--depth", "3",
                            "--mat", "1", "--denoise", "--bend", str(bend), "--out", str(tmp_path / f"{name}.pfm"), "--raw", str(raw)] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("reprojected through the previous pose" in r.stdout) == (name == "motion"), r.stdout
        cpp[name] = np.fromfile(raw, np.float32).reshape(H, W, 4)
    libm = C.CDLL("libm.so.6")
    libm.sinf.restype = libm.cosf.restype = C.c_float
    libm.sinf.argtypes = libm.cosf.argtypes = [C.c_float]
    scene = pkg.Scene.cornell()
    d = scene.desc
    P = positions_of(d)
    v3 = lambda ptr: np.ctypeslib.as_array(ptr, shape=(d.numVertices, 3)).astype(F).copy()
    Wt, ids, pivot = _bend_rig(P)
    vp = pkg.camera_view_proj((278.0, 273.0, -800.0), (278.0, 273.0, 0.0), (0.0, 1.0, 0.0), 33.6, 24.0, W / H, 0.1, 1000.0)
    flags = A.BMFR_PREPROCESS | A.BMFR_POSTPROCESS
    for name in ("motion", "plain"):
        pipe = pkg.FramePipeline(scene, W, H, max_depth=3, mat_index=1, accum_limit=100, motion=(name == "motion"))
        pipe.set_skin(P, Wt, ids, 4, v3(d.normals), v3(d.bitangents) if d.bitangents else None)
        for k in range(frames):
            bones, nbones = _bend_bones(libm, bend, k, pivot)
            pipe.update_skinned(bones, nbones)
            pipe.render_frame(accumulate=True)
            p = _params(pkg, k, flags, vp)
            if name == "motion":
                pipe.ctx.bmfr_execute_motion(p, pipe.gb, _ptr(pipe.prev_position), _ptr(pipe.output), pipe._stream_ptr())
            else:
                pipe.ctx.bmfr_execute(p, pipe.gb, _ptr(pipe.output), pipe._stream_ptr())
        torch.cuda.synchronize()
        py = pipe.output.cpu().numpy()
        assert np.array_equal(cpp[name].view(np.uint32), py.view(np.uint32)), (name, np.abs(cpp[name] - py).max())
        pipe.close()
    scene.close()
