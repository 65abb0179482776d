"""GPU tests of bdpt_trace_rays (csrc/trace_rays.hip): a caller's rays in device memory against the scene.  Every answer is
compared bit for bit — prim exactly, t / u / v as uint32 — with oracle_trace (its tree and, on a subset, its brute-force
scan) and with bdpt_test_trace on the same context."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import _random_rays
from test_refit_cpu import deform, moved_desc, positions_of

pytestmark = pytest.mark.gpu

MODES = ("closest", "closest_cull_back", "any")


def _to_bdpt(r):
    """oracle / test-hook layout (org, dir, tmin, tmax) -> bdpt_ray (org, tmin, dir, tmax)"""
    return np.ascontiguousarray(np.concatenate([r[:, 0:3], r[:, 6:7], r[:, 3:6], r[:, 7:8]], axis=1), np.float32)


def _gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _as_prim_tuv(res, mode):
    """trace_rays' answer in the oracle's form: prim (-1 miss; 0 = occluded for "any") and t / u / v"""
    if mode == "any":
        vis = res.cpu().numpy() if hasattr(res, "cpu") else res
        assert set(np.unique(vis)) <= {0, 1}
        return np.where(vis == 1, -1, 0).astype(np.int32), np.zeros((vis.shape[0], 3), np.float32)
    tuv, prim = res
    if hasattr(tuv, "cpu"):
        tuv, prim = tuv.cpu().numpy(), prim.cpu().numpy()
    return prim.astype(np.int32), np.ascontiguousarray(tuv, np.float32)


def _trace_device(ctx, rays, mode, stream=None):
    import torch
    res = ctx.trace_rays(_gpu(_to_bdpt(rays)), mode, stream=stream)
    torch.cuda.synchronize()
    return _as_prim_tuv(res, mode)


def _oracle(lib, osc, rays, mode, flags=0, n=None):
    n = rays.shape[0] if n is None else n
    po = np.zeros(n, np.int32)
    to = np.zeros((n, 3), np.float32)
    rays = np.ascontiguousarray(rays, np.float32)
    lib.oracle_trace(osc, rays.ctypes.data, n, MODES.index(mode), flags, po.ctypes.data, to.ctypes.data)
    return po, to


def _assert_same(prim, tuv, po, to, what):
    n = po.shape[0]
    assert np.array_equal(prim[:n], po), (what, int((prim[:n] != po).sum()))
    assert np.array_equal(tuv[:n].view(np.uint32), to.view(np.uint32)), (what, int((tuv[:n] != to).any(axis=1).sum()))


def _check_all(ctx, lib, osc, rays, mode, brute):
    """device path == oracle tree == oracle brute force (first `brute` rays) == bdpt_test_trace"""
    prim, tuv = _trace_device(ctx, rays, mode)
    _assert_same(prim, tuv, *_oracle(lib, osc, rays, mode), (mode, "tree"))
    if brute:
        _assert_same(prim, tuv, *_oracle(lib, osc, rays, mode, 1, brute), (mode, "brute"))
    hp, ht = ctx.test_trace(rays, MODES.index(mode))
    _assert_same(prim, tuv, hp, ht, (mode, "bdpt_test_trace"))
    return prim


def _scene_rays(rng, desc, n, frac_short=0.5):
    p = positions_of(desc)
    lo, hi = p.min(axis=0), p.max(axis=0)
    ext = float(np.max(hi - lo))
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[: n // 8] *= rng.uniform(0.1, 5.0, (n // 8, 1)).astype(np.float32)
    tmin = np.full((n, 1), 1e-4 * ext, np.float32)
    tmax = np.full((n, 1), 1e38, np.float32)
    k = int(n * frac_short)
    tmax[:k] = rng.uniform(0.01, 0.3, (k, 1)).astype(np.float32) * ext
    return np.concatenate([o, d, tmin, tmax], axis=1).astype(np.float32), ext


@pytest.mark.parametrize("ntri,edge", [(1, 0.9), (3, 0.8), (500, 0.3), (20000, 0.05)])
def test_soups_match_oracle_and_test_hook(pkg, ob, gpu_ctx, ntri, edge):
    scene = pkg.Scene.soup(7 + ntri, ntri, edge)
    gpu_ctx.set_scene(scene.desc)
    lib = ob.load_oracle(pkg.abi)
    osc = lib.oracle_scene_create(C.byref(scene.desc))
    rng = np.random.default_rng(100 + ntri)
    n = 8192
    rays = _random_rays(rng, n, -0.5, 1.5)
    rays[0, 3:6] = 0.0     # zero direction
    rays[1, 3:6] = np.nan  # NaN direction
    rays[2, 7] = 0.0       # tmax <= tmin
    rays[3, 0] = np.nan    # NaN origin
    for mode in MODES:
        prim = _check_all(gpu_ctx, lib, osc, rays, mode, n if ntri <= 500 else 1024)
        assert (prim[:4] == -1).all()
        assert (prim >= 0).sum() > 0 or ntri < 10
    lib.oracle_scene_destroy(osc)
    scene.close()


@pytest.mark.parametrize("which", ["atrium", "courtyard"])
def test_large_scenes_match_oracle(pkg, ob, gpu_ctx, which):
    """The 262 k-triangle atrium and the courtyard with alpha-masked foliage, as bdpt_set_scene builds them."""
    scene = pkg.Scene.atrium(1, 262144) if which == "atrium" else pkg.Scene.courtyard(1, 262144)
    gpu_ctx.set_scene(scene.desc)
    lib = ob.load_oracle(pkg.abi)
    osc = lib.oracle_scene_create(C.byref(scene.desc))
    rays, _ = _scene_rays(np.random.default_rng(11), scene.desc, 16384)
    for mode in MODES:
        prim = _check_all(gpu_ctx, lib, osc, rays, mode, 128)
        assert 0 < (prim >= 0).sum() < len(prim)
    lib.oracle_scene_destroy(osc)
    scene.close()


def test_stacks_beyond_the_lds_rows(pkg, ob, gpu_ctx):
    """The 300 000-triangle overlapping soup: descents deeper than the kernel's LDS stack rows use the overflow area."""
    scene = pkg.Scene.soup(99, 300000, 0.9)
    gpu_ctx.set_scene(scene.desc)
    lib = ob.load_oracle(pkg.abi)
    osc = lib.oracle_scene_create(C.byref(scene.desc))
    rng = np.random.default_rng(5)
    n = 20000
    rays = _random_rays(rng, n, -0.5, 1.5)
    rays[:, 6] = 0.0
    rays[:, 7] = rng.uniform(1e-6, 3e-5, n).astype(np.float32)
    _, deepest = gpu_ctx.test_trace_shadow(rays[:4096])
    assert deepest > 24, deepest  # these rays do go beyond the LDS rows
    for mode in ("closest", "any"):
        prim = _check_all(gpu_ctx, lib, osc, rays, mode, 64)
        assert 0 < (prim >= 0).sum() < n
    lib.oracle_scene_destroy(osc)
    scene.close()


def test_per_ray_tmin(pkg, ob, gpu_ctx):
    """tmin varies within one batch (the pass's any-hit kernel takes one tmin per launch): the same segment with several
    tmin values gets the answer of each."""
    scene = pkg.Scene.atrium(2, 20000)
    gpu_ctx.set_scene(scene.desc)
    lib = ob.load_oracle(pkg.abi)
    osc = lib.oracle_scene_create(C.byref(scene.desc))
    rng = np.random.default_rng(21)
    base, ext = _scene_rays(rng, scene.desc, 2048, frac_short=0.0)
    base[:, 7] = 0.5 * ext
    rays = np.concatenate([base] * 4)
    rays[:, 6] = np.repeat(np.array([0.0, 0.05, 0.15, 0.3], np.float32) * ext, 2048)
    for mode in MODES:
        prim = _check_all(gpu_ctx, lib, osc, rays, mode, 256)
        by_tmin = prim.reshape(4, 2048)
        assert (by_tmin[0] != by_tmin[3]).any()  # the answers do depend on tmin
    lib.oracle_scene_destroy(osc)
    scene.close()


def test_ambient_occlusion_rays_from_a_rendered_frame(pkg, ob):
    """Ambient-occlusion rays built from a frame's WorldPosition / WorldNormal channels (what aoTracing.rt.hlsl traces),
    through FramePipeline.trace_rays on the pipeline's stream."""
    import torch
    scene = pkg.Scene.atrium(1, 30000)
    pipe = pkg.FramePipeline(scene, 160, 90, max_depth=3)
    pipe.render_frame()
    torch.cuda.synchronize()
    pos = pipe.channels["WorldPosition"].cpu().numpy().reshape(-1, 4)
    nrm = pipe.channels["WorldNormal"].float().cpu().numpy().reshape(-1, 4)[:, :3]
    ok = (np.linalg.norm(nrm, axis=1) > 0.5) & np.isfinite(pos).all(axis=1)
    assert ok.sum() > 1000
    o, nv = pos[ok, :3], nrm[ok] / np.linalg.norm(nrm[ok], axis=1, keepdims=True)
    rng = np.random.default_rng(3)
    d = rng.normal(size=o.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = np.where((d * nv).sum(axis=1, keepdims=True) < 0, -d, d) + nv  # hemisphere around the normal, cosine-leaning
    ext = float(np.ptp(positions_of(scene.desc), axis=0).max())
    rays = np.concatenate([o, d, np.full((len(o), 1), 1e-3 * ext), np.full((len(o), 1), 0.1 * ext)], axis=1).astype(np.float32)
    lib = ob.load_oracle(pkg.abi)
    osc = lib.oracle_scene_create(C.byref(scene.desc))
    vis = pipe.trace_rays(_gpu(_to_bdpt(rays)), "any")
    torch.cuda.synchronize()
    prim, tuv = _as_prim_tuv(vis, "any")
    _assert_same(prim, tuv, *_oracle(lib, osc, rays, "any"), "ao")
    assert 0 < (prim >= 0).sum() < len(prim)
    lib.oracle_scene_destroy(osc)
    pipe.close()
    scene.close()


def test_device_count(pkg, ob, gpu_ctx):
    """count = M < N traces the first M rays and leaves the outputs beyond them as they were; M = 0 writes nothing;
    M > N is clamped to N."""
    import torch
    scene = pkg.Scene.atrium(2, 20000)
    gpu_ctx.set_scene(scene.desc)
    rays, _ = _scene_rays(np.random.default_rng(4), scene.desc, 5000)
    rt = _gpu(_to_bdpt(rays))
    n = rays.shape[0]
    full_c = _trace_device(gpu_ctx, rays, "closest")
    full_a = _trace_device(gpu_ctx, rays, "any")
    for m in (1234, 0, n + 100):
        cnt = torch.tensor([m], dtype=torch.int32, device="cuda")
        hits = torch.full((n, 4), -7, dtype=torch.int32, device="cuda")
        vis = torch.full((n,), 0xAB, dtype=torch.uint8, device="cuda")
        gpu_ctx.trace_rays(rt, "closest", out=hits, count=cnt)
        gpu_ctx.trace_rays(rt, "any", out=vis, count=cnt.view(torch.uint32))
        torch.cuda.synchronize()
        k = min(m, n)
        h = hits.cpu().numpy()
        assert (h[k:] == -7).all() and (vis.cpu().numpy()[k:] == 0xAB).all()
        assert np.array_equal(h[:k, 3], full_c[0][:k])
        assert np.array_equal(h[:k, :3].view(np.uint32), full_c[1][:k].view(np.uint32))
        assert np.array_equal(_as_prim_tuv(vis[:k], "any")[0], full_a[0][:k])
    scene.close()


def test_after_a_device_update_on_the_same_stream(pkg, ob):
    """update_geometry (device path) then trace_rays on one stream: the answers are the moved scene's."""
    import torch
    scene = pkg.Scene.atrium(5, 12000)
    pipe = pkg.FramePipeline(scene, 64, 36, max_depth=3)
    p1 = deform(positions_of(scene.desc), seed=8, amp=0.02)
    rays, _ = _scene_rays(np.random.default_rng(9), scene.desc, 8192)
    lib = ob.load_oracle(pkg.abi)
    desc1 = moved_desc(pkg, scene.desc, p1)
    osc = lib.oracle_scene_create(C.byref(desc1))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        pipe.render_frame()
        pipe.update_geometry(_gpu(p1))
        res = {m: pipe.trace_rays(_gpu(_to_bdpt(rays)), m) for m in MODES}
    torch.cuda.synchronize()
    for m in MODES:
        prim, tuv = _as_prim_tuv(res[m], m)
        _assert_same(prim, tuv, *_oracle(lib, osc, rays, m), (m, "moved"))
    lib.oracle_scene_destroy(osc)
    pipe.close()
    scene.close()


def test_captured_in_a_graph(pkg):
    """One trace_rays captured into a graph (one stream, no branches) with the ray tensor rewritten in place before the
    replay equals a direct call on the new rays."""
    import torch
    scene = pkg.Scene.atrium(5, 12000)
    ctx = pkg.Context(0)
    ctx.set_scene(scene.desc)
    rng = np.random.default_rng(12)
    r0, _ = _scene_rays(rng, scene.desc, 6000)
    r1, _ = _scene_rays(rng, scene.desc, 6000)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        st = C.c_void_p(side.cuda_stream)
        rays = _gpu(_to_bdpt(r0))
        out = torch.zeros((6000, 4), dtype=torch.float32, device="cuda")
        ref = torch.zeros((6000, 4), dtype=torch.float32, device="cuda")
        ctx.trace_rays(_gpu(_to_bdpt(r1)), out=ref, stream=st)  # direct call on the new rays
        graph = torch.cuda.CUDAGraph()
        graph.capture_begin()
        ctx.trace_rays(rays, out=out, stream=st)
        graph.capture_end()
    torch.cuda.synchronize()
    assert not out.any()  # captured, not run
    rays.copy_(_gpu(_to_bdpt(r1)))
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
    assert (ref.view(torch.int32)[:, 3] >= 0).any()
    again = torch.zeros_like(out)
    ctx.trace_rays(rays, out=again)  # a direct call after the replays
    torch.cuda.synchronize()
    assert torch.equal(again.view(torch.int32), ref.view(torch.int32))
    del graph
    ctx.close()
    scene.close()


def test_frames_are_unchanged_by_a_trace(pkg):
    """frame, trace, frame gives the image of two frames without the trace, bit for bit; the counters the frame left are
    unchanged by the trace."""
    import torch
    scene = pkg.Scene.atrium(3, 20000)
    rays, _ = _scene_rays(np.random.default_rng(2), scene.desc, 30000)
    imgs = []
    for with_trace in (True, False):
        pipe = pkg.FramePipeline(scene, 96, 54, max_depth=4, flags=pkg.abi.PARAM_COUNTERS)
        pipe.render_frame()
        if with_trace:
            before = pipe.ctx.counters().as_dict()
            times = pipe.ctx.stage_times()
            for m in MODES:
                pipe.trace_rays(_gpu(_to_bdpt(rays)), m)
            torch.cuda.synchronize()
            assert pipe.ctx.counters().as_dict() == before
            assert pipe.ctx.stage_times() == times
        pipe.render_frame()
        torch.cuda.synchronize()
        imgs.append(pipe.output.cpu().numpy())
        pipe.close()
    assert np.array_equal(imgs[0].view(np.uint32), imgs[1].view(np.uint32))
    scene.close()


def test_a_context_never_resized_can_trace(pkg, ob):
    scene = pkg.Scene.cornell()
    ctx = pkg.Context(0)
    ctx.set_scene(scene.desc)
    lib = ob.load_oracle(pkg.abi)
    osc = lib.oracle_scene_create(C.byref(scene.desc))
    rays, _ = _scene_rays(np.random.default_rng(6), scene.desc, 4096)
    for m in MODES:
        _check_all(ctx, lib, osc, rays, m, 4096)
    # host arrays: copied, traced, synchronised, returned as numpy
    tuv, prim = ctx.trace_rays(_to_bdpt(rays))
    assert isinstance(prim, np.ndarray)
    _assert_same(prim, tuv, *_oracle(lib, osc, rays, "closest"), "host path")
    lib.oracle_scene_destroy(osc)
    ctx.close()
    scene.close()


def test_error_cases_through_the_c_abi(pkg):
    import torch
    lib = pkg.load_library()
    scene = pkg.Scene.cornell()
    ctx = pkg.Context(0)
    rays = _gpu(_to_bdpt(_scene_rays(np.random.default_rng(1), scene.desc, 256)[0]))
    hits = torch.full((256, 4), -7, dtype=torch.int32, device="cuda")
    vis = torch.full((256,), 0xAB, dtype=torch.uint8, device="cuda")
    cnt = torch.tensor([256], dtype=torch.int32, device="cuda")

    def call(h=ctx._h, rays_p=rays.data_ptr(), n=256, mode=0, count=None, hits_p=hits.data_ptr(), vis_p=vis.data_ptr(), desc=True):
        d = pkg.abi.TraceDesc()
        d.rays, d.numRays, d.mode, d.numRaysDevice, d.hits, d.visible = rays_p, n, mode, count, hits_p, vis_p
        return lib.bdpt_trace_rays(h, C.byref(d) if desc else None, None)

    assert call() == -2                                    # BDPT_E_STATE: no scene
    ctx.set_scene(scene.desc)
    assert call(h=None) == -1                              # NULL context
    assert call(desc=False) == -1                          # NULL desc
    assert call(mode=3) == -1                              # unknown mode
    assert call(rays_p=None) == -1                         # missing rays
    assert call(rays_p=rays.data_ptr() + 4) == -1          # misaligned rays
    assert call(hits_p=None) == -1                         # closest without hits
    assert call(mode=1, hits_p=hits.data_ptr() + 8) == -1  # misaligned hits
    assert call(mode=2, vis_p=None) == -1                  # any without visible
    assert call(count=cnt.data_ptr() + 2) == -1            # misaligned count
    assert call(n=0, rays_p=None, hits_p=None, vis_p=None) == 0  # nothing to do
    torch.cuda.synchronize()
    assert (hits.cpu().numpy() == -7).all() and (vis.cpu().numpy() == 0xAB).all()  # nothing was enqueued
    assert call(count=cnt.data_ptr()) == 0 and call(mode=2, count=cnt.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (hits.cpu().numpy()[:, 3] != -7).all() and (vis.cpu().numpy() <= 1).all()
    ctx.close()
    scene.close()
