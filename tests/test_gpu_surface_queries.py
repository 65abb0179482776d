"""GPU tests of the surface queries (csrc/surface_query.hip): bdpt_camera_rays, bdpt_shade_hits and bdpt_bsdf_query.
Everything is compared bit for bit: with the G-buffer pass (camera rays -> trace_rays -> shade_hits is bdpt_gbuffer_execute
split in three), with numpy restatements of the ray and the shading geometry (test_surface_queries_cpu, rehearsed there
against the CPU oracle), and with oracle_bsdf / bdpt_test_bsdf."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import _random_rays
from test_refit_cpu import deform, moved_desc, positions_of
from test_surface_queries_cpu import pinhole_rays, shade_geometry

pytestmark = pytest.mark.gpu

W, H = 96, 64


def _gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u32(t):
    return (t.cpu().numpy() if hasattr(t, "cpu") else t).view(np.uint32)


def _half(lib, a):
    a = np.ascontiguousarray(a, np.float32)
    out = np.zeros_like(a)
    lib.oracle_half_round(a.ctypes.data, a.size, out.ctypes.data)
    return out


def _split_path(ctx, gp, st=None, normal_map=True):
    """camera rays -> closest hit with back faces culled -> shading: (rays, hits, surfaces) GPU tensors"""
    import torch
    rays = ctx.camera_rays(gp, W, H, stream=st)
    hits = torch.empty((W * H, 4), dtype=torch.float32, device="cuda")
    ctx.trace_rays(rays, "closest_cull_back", out=hits, stream=st)
    surf = ctx.shade_hits(rays, hits, normal_map=normal_map, stream=st)
    return rays, hits, surf


def _assert_gbuffer_identity(ob, pkg, pipe, surf, thin_lens=False):
    """surf (W*H, 24) against the pipeline's G-buffer channels"""
    lib = ob.load_oracle(pkg.abi)
    s = surf.cpu().numpy()
    prim = s.view(np.int32)[:, 23]
    pos = pipe.channels["WorldPosition"].cpu().numpy().reshape(-1, 4)
    ch = {n: pipe.channels[n].float().cpu().numpy().reshape(-1, 4) for n in
          ("WorldNormal", "MaterialDiffuse", "MaterialSpecRough", "MaterialExtraParams", "Emissive")}
    miss = prim == -1
    assert np.array_equal(miss, pos[:, 3] == 0) and (prim >= -1).all()
    hit = ~miss
    assert np.array_equal(_u32(pos[hit, :3]), _u32(s[hit, 0:3])) and (pos[hit, 3] == 1).all()
    z = np.zeros((int(hit.sum()), 1), np.float32)
    expect = {
        "MaterialDiffuse": s[hit][:, 12:16],
        "MaterialSpecRough": np.concatenate([s[hit][:, 16:19], s[hit][:, 7:8]], axis=1),
        "MaterialExtraParams": np.concatenate([s[hit][:, 11:12], z, z, z], axis=1),
        "Emissive": np.concatenate([s[hit][:, 20:23], z], axis=1),
    }
    if not thin_lens:
        expect["WorldNormal"] = np.concatenate([s[hit][:, 4:7], s[hit][:, 3:4]], axis=1)
    for name, e in expect.items():
        assert np.array_equal(_u32(ch[name][hit]), _u32(_half(lib, e))), name
    # misses: every float 0, material 0xffffffff
    assert (_u32(s[miss][:, :19]) == 0).all() and (_u32(s[miss][:, 20:23]) == 0).all()
    assert (s.view(np.uint32)[miss, 19] == 0xFFFFFFFF).all()
    return hit


SCENES = {
    "cornell": lambda pkg: pkg.Scene.cornell(),
    "atrium": lambda pkg: pkg.Scene.atrium(1, 40000),
    "courtyard": lambda pkg: pkg.Scene.courtyard(1, 60000),
}


@pytest.mark.parametrize("which", list(SCENES))
def test_split_path_equals_the_gbuffer_pass(pkg, ob, which):
    """camera_rays -> trace_rays(closest_cull_back) -> shade_hits(normal_map=True) is bdpt_gbuffer_execute of the same
    params: pinhole with and without jitter at two frame counters, and thin lens (all but WorldNormal, whose V and
    distance are taken from the camera position, not the lens point)."""
    import torch
    scene = SCENES[which](pkg)
    pipe = pkg.FramePipeline(scene, W, H, max_depth=3)
    st = pipe._stream_ptr()
    for jitter in (True, False):
        for frame in (0xdeadbeef, 0xdeadbef5):
            for thin in (False, True):
                if thin and not jitter:
                    continue
                pipe.use_jitter, pipe.gbuffer_frame = jitter, frame
                gp = pipe.gbuffer_params()
                gp.useThinLens = 1 if thin else 0
                rays, _, surf = _split_path(pipe.ctx, gp, st)
                pipe.ctx.gbuffer_execute(gp, pipe.gb, st)
                torch.cuda.synchronize()
                hit = _assert_gbuffer_identity(ob, pkg, pipe, surf, thin_lens=thin)
                assert hit.sum() > 0
                if not thin:  # the rays themselves: primaryRay's pinhole branch restated in numpy
                    ref = pinhole_rays(pipe.cam, W, H, gp.pixelJitter)
                    assert np.array_equal(_u32(rays), ref.view(np.uint32)), (which, jitter, frame)
    pipe.close()
    scene.close()


def _without_normal_maps(pkg, desc):
    """a copy of desc whose materials have no normal map (kept alive through the returned tuple)"""
    n = int(desc.numMaterials)
    mats = (pkg.abi.Material * n)()
    for i in range(n):
        mats[i] = desc.materials[i]
        mats[i].texNormal = -1
    d = pkg.abi.SceneDesc()
    C.pointer(d)[0] = desc
    d.materials = C.cast(mats, C.POINTER(pkg.abi.Material))
    return d, mats


def test_normal_map_flag(pkg):
    """On the atrium, normal_map=False (the walk's shading) differs from True on some hits and equals True on the same
    scene with every normal map removed."""
    import torch
    scene = pkg.Scene.atrium(1, 40000)
    pipe = pkg.FramePipeline(scene, W, H, max_depth=3)
    gp = pipe.gbuffer_params()
    rays, hits, with_map = _split_path(pipe.ctx, gp)
    no_map = pipe.ctx.shade_hits(rays, hits, normal_map=False)
    bare_desc, keep = _without_normal_maps(pkg, scene.desc)
    bare = pkg.Context(0)
    bare.set_scene(bare_desc)
    torch.cuda.synchronize()
    bare_map = bare.shade_hits(rays, hits, normal_map=True)
    torch.cuda.synchronize()
    a, b, c = (_u32(t) for t in (with_map, no_map, bare_map))
    hit = a.view(np.int32)[:, 23] >= 0
    assert (a[hit] != b[hit]).any(axis=1).sum() > 0  # the normal maps are live
    assert np.array_equal(b, c)
    assert np.array_equal(np.delete(a, [4, 5, 6], axis=1), np.delete(b, [4, 5, 6], axis=1))  # only N differs
    bare.close()
    pipe.close()
    scene.close()
    del keep


@pytest.mark.parametrize("which", ["soup", "cornell"])
def test_geometry_on_random_rays(pkg, ob, gpu_ctx, which):
    """Random rays (closest hit): posW, dist, V and the unmapped N equal the numpy restatement of shadeHit."""
    import torch
    scene = pkg.Scene.soup(11, 5000, 0.1) if which == "soup" else pkg.Scene.cornell()
    gpu_ctx.set_scene(scene.desc)
    lo, hi = (-0.5, 1.5) if which == "soup" else (-1.0, 1.0)
    p = positions_of(scene.desc)
    if which == "cornell":
        lo, hi = float(p.min()), float(p.max())
    r = _random_rays(np.random.default_rng(8), 20000, lo, hi)
    rays = np.ascontiguousarray(np.concatenate([r[:, 0:3], r[:, 6:7], r[:, 3:6], r[:, 7:8]], axis=1), np.float32)
    rt = _gpu(rays)
    hits = torch.empty((len(rays), 4), dtype=torch.float32, device="cuda")
    gpu_ctx.trace_rays(rt, "closest", out=hits)
    s = gpu_ctx.shade_hits(rt, hits, normal_map=False)
    s2 = gpu_ctx.shade_hits(rt, hits, normal_map=True)
    torch.cuda.synchronize()
    s, h = s.cpu().numpy(), hits.cpu().numpy()
    prim = h.view(np.int32)[:, 3]
    hit = prim >= 0
    assert 0 < hit.sum() < len(prim)
    assert np.array_equal(s.view(np.int32)[:, 23], prim)
    posW, N, V, dist = shade_geometry(scene.desc, rays[hit, 0:3], prim[hit], h[hit, 1], h[hit, 2])
    for cols, ref, name in (((0, 3), posW, "posW"), ((4, 7), N, "N"), ((8, 11), V, "V")):
        assert np.array_equal(s[hit, cols[0]:cols[1]].view(np.uint32), ref.view(np.uint32)), name
    assert np.array_equal(s[hit, 3].view(np.uint32), dist.view(np.uint32))
    assert np.array_equal(s.view(np.uint32), _u32(s2))  # no normal maps in these scenes
    # host arrays: copied, shaded, synchronised, returned as numpy
    host = gpu_ctx.shade_hits(rays, h, normal_map=False)
    assert isinstance(host, np.ndarray) and np.array_equal(host.view(np.uint32), s.view(np.uint32))
    scene.close()


def _bsdf_records(rng, n):
    """random bdpt_surface records (some misses) and the matching 20-float bdpt_test_bsdf records"""
    def unit(k):
        v = rng.normal(size=(k, 3))
        return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)

    Nn, V, L = unit(n), unit(n), unit(n)
    V = np.where((np.sum(Nn * V, axis=1, keepdims=True) < 0) & (rng.uniform(size=(n, 1)) < 0.9), -V, V)
    surf = np.zeros((n, 24), np.float32)
    surf[:, 4:7], surf[:, 8:11] = Nn, V
    surf[:, 7] = rng.uniform(0.08, 1, n)
    surf[:, 12:15] = rng.uniform(0, 1, (n, 3))
    surf[:, 16:19] = rng.uniform(0, 1, (n, 3))
    surf[:8, 12:15] = surf[:8, 16:19] = 0.0  # black materials
    prim = rng.integers(0, 1000, n).astype(np.int32)
    prim[rng.uniform(size=n) < 0.05] = -1
    surf.view(np.int32)[:, 23] = prim
    seeds = rng.integers(0, 2**32, n, dtype=np.uint32)
    is_spec = rng.integers(0, 2, n).astype(np.float32)
    rec = np.zeros((n, 20), np.float32)
    rec[:, 0:3], rec[:, 3:6], rec[:, 6:9] = Nn, V, L
    rec[:, 9:12], rec[:, 12:15] = surf[:, 12:15], surf[:, 16:19]
    rec[:, 15] = surf[:, 7] * surf[:, 7]
    rec[:, 16] = is_spec
    rec[:, 17] = seeds.view(np.float32)
    dirs = np.ascontiguousarray(np.concatenate([L, is_spec[:, None]], axis=1), np.float32)
    return surf, seeds, dirs, rec, prim


def _same(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("mat", [0, 1])
@pytest.mark.parametrize("from_lobe", [False, True])
def test_bsdf_parity(pkg, ob, gpu_ctx, mat, from_lobe):
    """sample_bsdf / eval_bsdf equal bdpt_test_bsdf and oracle_bsdf on the same inputs; miss records give zeros."""
    import torch
    scene = pkg.Scene.cornell()
    gpu_ctx.set_scene(scene.desc)
    n = 20000
    surf, seeds, dirs, rec, prim = _bsdf_records(np.random.default_rng(31 + mat + 2 * from_lobe), n)
    st = _gpu(surf)
    samp = gpu_ctx.sample_bsdf(st, _gpu(seeds), mat_index=mat, from_lobe=from_lobe)
    vals = gpu_ctx.eval_bsdf(st, _gpu(dirs), mat_index=mat)
    torch.cuda.synchronize()
    samp, vals = samp.cpu().numpy(), vals.cpu().numpy()
    code = mat | (2 if from_lobe else 0)
    hook = gpu_ctx.test_bsdf(rec, code)
    ref = np.zeros_like(hook)
    ob.load_oracle(pkg.abi).oracle_bsdf(np.ascontiguousarray(rec).ctypes.data, n, code, ref.ctypes.data)
    assert _same(hook, ref).all()
    ok = prim >= 0
    assert _same(samp[ok, 0:3], hook[ok, 3:6]).all() and _same(samp[ok, 3], hook[ok, 6]).all()
    assert _same(samp[ok, 4:7], hook[ok, 0:3]).all()
    assert np.array_equal(samp.view(np.uint32)[ok, 7], hook[ok, 7].astype(np.uint32))
    assert _same(vals[ok, 0:3], hook[ok, 8:11]).all() and (vals[:, 3] == 0).all()
    assert (samp[~ok].view(np.uint32) == 0).all() and (vals[~ok].view(np.uint32) == 0).all()
    if mat == 0:
        assert (samp[ok, 3] == 0).sum() > 0  # samples below the surface: pdf 0
        assert ((samp.view(np.uint32)[ok, 7] == 1).sum() > 0) == from_lobe
    scene.close()


def test_device_counts(pkg, gpu_ctx):
    """count = M < N: the first M items are written, as without a count, and the rest are left as they were."""
    import torch
    scene = pkg.Scene.atrium(2, 20000)
    pipe = pkg.FramePipeline(scene, W, H, max_depth=3)
    ctx = pipe.ctx
    rays, hits, full = _split_path(ctx, pipe.gbuffer_params())
    seeds = _gpu(np.arange(W * H, dtype=np.uint32) * np.uint32(2654435761))
    full_s = ctx.sample_bsdf(full, seeds)
    dirs = torch.cat([full_s[:, 0:3], full_s[:, 7:8].view(torch.int32).float()], dim=1).contiguous()
    full_e = ctx.eval_bsdf(full, dirs)
    n = W * H
    for m in (1000, 0, n + 5):
        cnt = torch.tensor([m], dtype=torch.int32, device="cuda")
        s = torch.full((n, 24), -7, dtype=torch.int32, device="cuda")
        a = torch.full((n, 8), -7, dtype=torch.int32, device="cuda")
        e = torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda")
        ctx.shade_hits(rays, hits, out=s, count=cnt)
        ctx.sample_bsdf(full, seeds, out=a, count=cnt.view(torch.uint32))
        ctx.eval_bsdf(full, dirs, out=e, count=cnt)
        torch.cuda.synchronize()
        k = min(m, n)
        for got, ref in ((s, full), (a, full_s), (e, full_e)):
            g = _u32(got)
            assert np.array_equal(g[:k], _u32(ref)[:k])
            assert (g[k:] == np.float32(-7.0).view(np.uint32)).all() or (g[k:].view(np.int32) == -7).all()
    pipe.close()
    scene.close()


def test_after_a_device_update_on_the_same_stream(pkg, ob):
    """update_geometry, then camera rays -> trace -> shade on one stream: the G-buffer identity holds for the moved
    scene (the refit rewrote the shading records)."""
    import torch
    scene = pkg.Scene.atrium(5, 12000)
    pipe = pkg.FramePipeline(scene, W, H, max_depth=3)
    p1 = deform(positions_of(scene.desc), seed=8, amp=0.02)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        st = pipe._stream_ptr()
        pipe.render_frame()
        before = pipe.shade_hits(*_split_path(pipe.ctx, pipe.gbuffer_params(), st)[:2])
        pipe.update_geometry(_gpu(p1))
        gp = pipe.gbuffer_params()
        _, _, surf = _split_path(pipe.ctx, gp, st)
        pipe.ctx.gbuffer_execute(gp, pipe.gb, st)
    torch.cuda.synchronize()
    _assert_gbuffer_identity(ob, pkg, pipe, surf)
    hit = _u32(surf).view(np.int32)[:, 23] >= 0
    assert not np.array_equal(_u32(surf)[hit, :3], _u32(before)[hit, :3])  # the scene did move
    # and the positions are the moved mesh's (restated from the moved vertices)
    s = surf.cpu().numpy()
    moved = moved_desc(pkg, scene.desc, p1)
    rays = pinhole_rays(pipe.cam, W, H, gp.pixelJitter)
    posW, _, _, _ = shade_geometry(moved, rays[hit, 0:3], s.view(np.int32)[hit, 23],
                                   *_hits_uv(pipe, rays, hit))
    assert np.array_equal(s[hit, 0:3].view(np.uint32), posW.view(np.uint32))
    pipe.close()
    scene.close()


def _hits_uv(pipe, rays, hit):
    import torch
    rt = _gpu(rays)
    h = torch.empty((len(rays), 4), dtype=torch.float32, device="cuda")
    pipe.ctx.trace_rays(rt, "closest_cull_back", out=h)
    torch.cuda.synchronize()
    h = h.cpu().numpy()
    return h[hit, 1], h[hit, 2]


def test_frames_are_unchanged_by_the_queries(pkg):
    """frame, queries, frame gives the image of two frames without the queries, bit for bit; counters and stage times
    the frame left are unchanged."""
    import torch
    scene = pkg.Scene.atrium(3, 20000)
    imgs = []
    for with_queries in (True, False):
        pipe = pkg.FramePipeline(scene, W, H, max_depth=4, flags=pkg.abi.PARAM_COUNTERS)
        pipe.ctx.enable_stage_timing(True)
        pipe.render_frame()
        if with_queries:
            torch.cuda.synchronize()
            before = pipe.ctx.counters().as_dict()
            times = pipe.ctx.stage_times()
            rays = pipe.camera_rays()
            hits = torch.empty((W * H, 4), dtype=torch.float32, device="cuda")
            pipe.trace_rays(rays, "closest", out=hits)
            surf = pipe.shade_hits(rays, hits)
            samp = pipe.sample_bsdf(surf, _gpu(np.arange(W * H, dtype=np.uint32)))
            pipe.eval_bsdf(surf, torch.cat([samp[:, 0:3], samp[:, 7:8]], dim=1).contiguous())
            torch.cuda.synchronize()
            assert pipe.ctx.counters().as_dict() == before
            assert pipe.ctx.stage_times() == times
        pipe.render_frame()
        torch.cuda.synchronize()
        imgs.append(pipe.output.cpu().numpy())
        pipe.close()
    assert np.array_equal(imgs[0].view(np.uint32), imgs[1].view(np.uint32))
    scene.close()


def test_error_cases_through_the_c_abi(pkg):
    import torch
    a = pkg.abi
    lib = pkg.load_library()
    scene = pkg.Scene.cornell()
    ctx = pkg.Context(0)
    n = 256
    rays = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    hits = torch.full((n, 4), -1, dtype=torch.int32, device="cuda")
    surf = torch.full((n, 24), -7, dtype=torch.int32, device="cuda")
    seeds = torch.zeros(n, dtype=torch.int32, device="cuda")
    out8 = torch.full((n, 8), -7, dtype=torch.int32, device="cuda")
    out4 = torch.full((n, 4), -7, dtype=torch.int32, device="cuda")
    gp = a.GBufferParams()

    def cam(h=ctx._h, w=16, hh=16, p=rays.data_ptr(), gpp=True):
        return lib.bdpt_camera_rays(h, C.byref(gp) if gpp else None, w, hh, p, None)

    def shade(h=ctx._h, r=rays.data_ptr(), hi=hits.data_ptr(), num=n, flags=0, cnt=None, out=surf.data_ptr(), desc=True):
        d = a.ShadeDesc()
        d.rays, d.hits, d.numHits, d.flags, d.numHitsDevice, d.surfaces = r, hi, num, flags, cnt, out
        return lib.bdpt_shade_hits(h, C.byref(d) if desc else None, None)

    def bsdf(h=ctx._h, s=surf.data_ptr(), num=n, mode=0, cnt=None, mat=0, flags=0, sd=seeds.data_ptr(), smp=out8.data_ptr(),
             dirs=out4.data_ptr(), vals=out4.data_ptr(), desc=True):
        d = a.BsdfDesc()
        d.surfaces, d.num, d.mode, d.numDevice, d.matIndex, d.flags = s, num, mode, cnt, mat, flags
        d.seeds, d.samples, d.dirs, d.values = sd, smp, dirs, vals
        return lib.bdpt_bsdf_query(h, C.byref(d) if desc else None, None)

    assert cam() == -2 and shade() == -2 and bsdf() == -2  # BDPT_E_STATE: no camera / no scene
    ctx.set_scene(scene.desc)
    ctx.set_camera(scene.camera(1.0))
    bad = [
        cam(h=None), cam(gpp=False), cam(w=0), cam(hh=0), cam(w=65536, hh=65536), cam(p=None), cam(p=rays.data_ptr() + 4),
        shade(h=None), shade(desc=False), shade(flags=2), shade(r=None), shade(r=rays.data_ptr() + 8), shade(hi=None),
        shade(hi=hits.data_ptr() + 4), shade(out=None), shade(out=surf.data_ptr() + 8), shade(cnt=seeds.data_ptr() + 2),
        bsdf(h=None), bsdf(desc=False), bsdf(mode=2), bsdf(mat=2), bsdf(flags=1), bsdf(s=None), bsdf(s=surf.data_ptr() + 4),
        bsdf(sd=None), bsdf(sd=seeds.data_ptr() + 2), bsdf(smp=None), bsdf(smp=out8.data_ptr() + 8), bsdf(mode=1, dirs=None),
        bsdf(mode=1, dirs=out4.data_ptr() + 4), bsdf(mode=1, vals=None), bsdf(mode=1, vals=out4.data_ptr() + 8),
        bsdf(cnt=seeds.data_ptr() + 1),
    ]
    assert all(rc == -1 for rc in bad), bad
    assert shade(num=0, r=None, hi=None, out=None) == 0 and bsdf(num=0, s=None, sd=None, smp=None) == 0
    torch.cuda.synchronize()
    assert (surf.cpu().numpy() == -7).all() and (out8.cpu().numpy() == -7).all() and (out4.cpu().numpy() == -7).all()
    assert shade() == 0 and bsdf() == 0 and bsdf(mode=1, dirs=torch.zeros((n, 4), device="cuda").data_ptr()) == 0
    torch.cuda.synchronize()
    assert (surf.cpu().numpy()[:, 23] == -1).all() and (out8.cpu().numpy() == 0).all() and (out4.cpu().numpy() == 0).all()
    ctx.close()
    scene.close()


def test_captured_loop(pkg):
    """camera rays, trace, shade, sample and an any-hit trace along the samples captured into one graph on one stream
    (no parallel branches): the replay equals the eager run, and capturing allocates nothing."""
    import torch
    scene = pkg.Scene.atrium(4, 20000)
    pipe = pkg.FramePipeline(scene, W, H, max_depth=3)
    ctx = pipe.ctx
    n = W * H
    ext = float(np.ptp(positions_of(scene.desc), axis=0).max())
    side = torch.cuda.Stream()
    seeds = _gpu(np.arange(n, dtype=np.uint32) * np.uint32(747796405))

    def buffers():
        b = dict(rays=torch.zeros((n, 8), device="cuda"), hits=torch.zeros((n, 4), device="cuda"),
                 surf=torch.zeros((n, 24), device="cuda"), samp=torch.zeros((n, 8), device="cuda"),
                 ray2=torch.zeros((n, 8), device="cuda"), vis=torch.zeros(n, dtype=torch.uint8, device="cuda"))
        b["ray2"][:, 3] = 1e-4 * ext
        b["ray2"][:, 7] = 0.25 * ext
        return b

    def loop(b, st):
        ctx.camera_rays(pipe.gbuffer_params(), W, H, out=b["rays"], stream=st)
        ctx.trace_rays(b["rays"], "closest", out=b["hits"], stream=st)
        ctx.shade_hits(b["rays"], b["hits"], out=b["surf"], stream=st)
        ctx.sample_bsdf(b["surf"], seeds, out=b["samp"], stream=st)
        b["ray2"][:, 0:3].copy_(b["surf"][:, 0:3])
        b["ray2"][:, 4:7].copy_(b["samp"][:, 0:3])
        ctx.trace_rays(b["ray2"], "any", out=b["vis"], stream=st)

    with torch.cuda.stream(side):
        st = C.c_void_p(side.cuda_stream)
        eager, cap = buffers(), buffers()
        loop(eager, st)
        side.synchronize()
        # torch's graphs keep an RNG seed and offset that the first capture of a process allocates: a graph of one in-place
        # op takes that, so that what the loop's capture allocates is the loop's own
        pad = torch.zeros(1, device="cuda")
        trivial = torch.cuda.CUDAGraph()
        trivial.capture_begin()
        pad.add_(1)
        trivial.capture_end()
        alloc = torch.cuda.memory_allocated()
        graph = torch.cuda.CUDAGraph()
        graph.capture_begin()
        loop(cap, st)
        graph.capture_end()
        assert torch.cuda.memory_allocated() == alloc  # the loop allocates nothing
    torch.cuda.synchronize()
    assert not cap["surf"].any()  # captured, not run
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for k in ("rays", "hits", "surf", "samp", "ray2", "vis"):
            assert torch.equal(cap[k].view(torch.uint8), eager[k].view(torch.uint8)), k
    vis = eager["vis"].cpu().numpy()
    assert 0 < (vis == 0).sum() < n
    del graph, trivial
    pipe.close()
    scene.close()
