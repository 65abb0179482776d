"""GPU tests of the piece-tight refit (bdpt_prepare(BDPT_PREPARE_REFIT_PIECES); csrc/refit.hip k_refit_regions and
k_refit_level_pieces): the device's records equal the host refit's bit for bit, images and ray queries after an update
equal those of a context built at the moved positions, skinned updates and captured updates go through the same refit,
and the mode keeps the conventions of include/bdpt.h "Animated scenes".  Three small scenes reach every branch: the
Cornell box (32 triangles, no pieces, a root-only tree), an atrium built with spatial splits and a courtyard with
alpha-clipped foliage (leaves of one and two references, nodes with fewer than four children, levels below and above
one 256-thread block)."""
import ctypes as C

import numpy as np
import pytest

import skin_numpy as sn
from test_gpu_configs import _assert_frame_equals_oracle
from test_gpu_refit import Moved, _frame, _torch_positions
from test_refit_cpu import HostTree, deform, moved_desc, positions_of

pytestmark = pytest.mark.gpu

SCENES = ["cornell", "atrium", "courtyard"]
CHANNELS = ("WorldPosition", "WorldNormal", "MaterialDiffuse", "MaterialSpecRough", "MaterialExtraParams", "Emissive")


def _scene(pkg, which, monkeypatch):
    """(scene, host budgets); the atrium's split budgets are in the environment for every bdpt_set_scene of the test"""
    if which == "cornell":
        return pkg.Scene.cornell(), (-1.0, -1.0, 1)
    if which == "atrium":
        monkeypatch.setenv("BDPT_SPLIT_BUDGET", "1")
        monkeypatch.setenv("BDPT_SPLIT_BUDGET_ALPHA", "4")
        return pkg.Scene.atrium(2, 6000), (1.0, 4.0, 1)
    return pkg.Scene.courtyard(2, 6000, 0.6), (-1.0, -1.0, 1)


def _host_pieces(pkg, scene, budgets):
    host = HostTree(pkg, scene.desc, *budgets)
    assert host.lib.bdpt_host_bvh_refit_pieces(host.h) == 0
    return host


@pytest.mark.parametrize("which", SCENES)
def test_device_piece_refit_equals_host_piece_refit(pkg, which, monkeypatch):
    """(1) Built pose and deform(p0), host pointers then device pointers: records and SAH cost equal the host's."""
    scene, budgets = _scene(pkg, which, monkeypatch)
    p0 = positions_of(scene.desc)
    ctx = pkg.Context(0)
    ctx.set_scene(scene.desc)
    host = _host_pieces(pkg, scene, budgets)
    assert ctx.recs_hash() == host.hash()  # (the same tree to start from)
    if which == "atrium":
        assert host.info.numReferences > scene.desc.numTriangles
    elif which == "courtyard":
        assert host.info.numReferences != scene.desc.numTriangles or host.info.numDropped > 0
    ctx.prepare(refit_pieces=True)
    ctx.prepare(refit_pieces=True)  # (again: nothing to do)
    assert ctx.recs_hash() == host.hash()  # (the prepare writes no record)
    plain = None
    if which == "cornell":
        plain = pkg.Context(0)
        plain.set_scene(scene.desc)
    updates = 0
    for pose in (p0, deform(p0)):
        host.refit(pose)
        for p in (pose, _torch_positions(pose)):
            ctx.update_geometry(p)
            updates += 1
            assert ctx.recs_hash() == host.hash()
            ri, hi = ctx.refit_info(), host.refit_info()
            assert ri.numUpdates == updates and ri.sahCost == hi.sahCost and ri.sahCostBuilt == hi.sahCostBuilt
        host.check()
        if plain is not None:
            plain.update_geometry(pose)
            assert plain.recs_hash() == ctx.recs_hash()
    if plain is not None:
        plain.close()
    host.close()
    ctx.close()
    scene.close()


def _parts(pkg, pipe):
    """One frame: (gp, p, G-buffer channels, splat words, image)"""
    import torch
    hip = C.CDLL("libamdhip64.so")
    gp, p = pipe.render_frame(extra_flags=pkg.abi.PARAM_DEFER_RESOLVE)
    torch.cuda.synchronize()
    chans = {ch: pipe.channels[ch].float().cpu().numpy().copy() for ch in CHANNELS}
    ptr, n64 = pipe.ctx.splat_buffer()
    spl = torch.empty(n64, dtype=torch.int64, device=pipe.dev)
    assert hip.hipMemcpy(C.c_void_p(spl.data_ptr()), C.c_void_p(ptr), C.c_size_t(n64 * 8), 3) == 0
    pipe.ctx.resolve(C.c_void_p(ptr), 0, C.c_void_p(pipe.output.data_ptr()), pipe._stream_ptr())
    torch.cuda.synchronize()
    return gp, p, chans, spl.cpu().numpy().copy(), pipe.output.cpu().numpy().copy()


@pytest.mark.parametrize("which", SCENES)
def test_frames_after_a_piece_refit_equal_a_rebuild_and_the_oracle(pkg, ob, which, monkeypatch):
    """(2) After the deforming update: G-buffer channels, splat buffer and frame equal a fresh context's (bdpt_set_scene at
    the moved positions) bit for bit, and the frame equals the oracle's on the moved description."""
    scene, _ = _scene(pkg, which, monkeypatch)
    W, H, D = (96, 54, 16) if which == "courtyard" else (64, 64, 4)
    p1 = deform(positions_of(scene.desc))
    d1 = moved_desc(pkg, scene.desc, p1)
    pipe = pkg.FramePipeline(scene, W, H, max_depth=D, mat_index=0)
    pipe.ctx.prepare(refit_pieces=True)
    _frame(pipe)
    pipe.update_geometry(_torch_positions(p1))
    gp, p, chans, spl, img = _parts(pkg, pipe)
    _assert_frame_equals_oracle(pkg, ob, Moved(scene, d1), pipe, gp, p, f"{which} piece refit")
    fresh = pkg.FramePipeline(Moved(scene, d1), W, H, max_depth=D, mat_index=0)
    fresh.gbuffer_frame, fresh.bdpt_frame = pipe.gbuffer_frame - 1, pipe.bdpt_frame - 1
    _, _, fchans, fspl, fimg = _parts(pkg, fresh)
    for ch in CHANNELS:
        assert np.array_equal(chans[ch].view(np.uint32), fchans[ch].view(np.uint32)), ch
    assert np.array_equal(spl, fspl)
    assert np.array_equal(img.view(np.uint32), fimg.view(np.uint32)), f"{(img != fimg).any(axis=-1).sum()} pixels differ"
    assert pipe.ctx.refit_info().numUpdates == 1
    fresh.close()
    pipe.close()
    scene.close()


def _query_rays(rng, n, lo, hi, tmax=None):
    """bdpt_ray layout: origin, tmin, direction, tmax"""
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3] = rng.uniform(lo, hi, (n, 3))
    r[:, 3] = 1e-4
    d = rng.normal(size=(n, 3))
    r[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    r[:, 7] = 1e38 if tmax is None else rng.uniform(0.1, tmax, n)
    return r


@pytest.mark.parametrize("which", SCENES)
def test_ray_queries_after_a_piece_refit_equal_a_rebuild(pkg, which, monkeypatch):
    """(3) bdpt_trace_rays, all three modes, 65 536 random rays: the refitted context answers as a fresh one does."""
    scene, _ = _scene(pkg, which, monkeypatch)
    p1 = deform(positions_of(scene.desc))
    d1 = moved_desc(pkg, scene.desc, p1)
    ctx = pkg.Context(0)
    ctx.set_scene(scene.desc)
    ctx.prepare(refit_pieces=True)
    ctx.update_geometry(p1)
    fresh = pkg.Context(0)
    fresh.set_scene(d1)
    rng = np.random.default_rng(7)
    lo, hi = p1.min(axis=0), p1.max(axis=0)
    n, hits = 65536, 0
    for mode in ("closest", "closest_cull_back", "any"):
        rays = _query_rays(rng, n, lo, hi, None if mode != "any" else float(np.max(hi - lo)) * 0.5)
        if mode == "any":
            assert np.array_equal(ctx.trace_rays(rays, mode), fresh.trace_rays(rays, mode))
        else:
            tuv, prim = ctx.trace_rays(rays, mode)
            ftuv, fprim = fresh.trace_rays(rays, mode)
            assert np.array_equal(prim, fprim)
            assert np.array_equal(np.ascontiguousarray(tuv).view(np.uint32), np.ascontiguousarray(ftuv).view(np.uint32))
            hits += int((prim >= 0).sum())
    assert hits > n // 4, "the sample must actually hit the moved scene"
    fresh.close()
    ctx.close()
    scene.close()


def test_skinned_update_refits_by_pieces(pkg, monkeypatch):
    """(4) update_skinned on a prepared context == update_geometry with bdpt_host_skin's positions on another."""
    scene, budgets = _scene(pkg, "atrium", monkeypatch)
    d = scene.desc
    nb = 5
    r = sn.scene_rig(d, 7, nb)
    a, b = pkg.Context(0), pkg.Context(0)
    for ctx in (a, b):
        ctx.set_scene(d)
        ctx.prepare(refit_pieces=True)
    a.set_skin(r["P"], r["W"], r["I"], nb, r["N"], r["B"])
    bones, nbones = sn.make_pose(11, nb, r["pivot"], r["extent"], angle=0.05, shift=0.005)
    rc, ep, _, _ = sn.host_skin(pkg.load_library(), pkg.abi, r["P"], r["W"], r["I"], bones)
    assert rc == 0
    a.update_skinned(_torch_positions(bones), _torch_positions(nbones))
    b.update_geometry(ep)
    assert a.recs_hash() == b.recs_hash()
    host = _host_pieces(pkg, scene, budgets)
    host.refit(ep)
    assert a.recs_hash() == host.hash()
    plain = pkg.Context(0)
    plain.set_scene(d)
    plain.update_geometry(ep)
    assert plain.recs_hash() != a.recs_hash()  # (the tree has pieces: the plain refit is another tree)
    for x in (plain, a, b):
        x.close()
    host.close()
    scene.close()


def test_piece_update_and_frame_captured_in_a_hip_graph(pkg, monkeypatch):
    """(5) A captured (device-pointer update, frame) on a prepared context, replayed twice with the position tensor
    rewritten in between: each replay equals the eager result."""
    import torch
    scene, _ = _scene(pkg, "atrium", monkeypatch)
    p0 = positions_of(scene.desc)
    poses = [_torch_positions(deform(p0, seed=8, amp=0.01)), _torch_positions(deform(p0, seed=9, amp=0.02))]
    pt = _torch_positions(p0)
    pipe = pkg.FramePipeline(scene, 64, 64, max_depth=4, mat_index=0)
    pipe.ctx.prepare(refit_pieces=True)
    side = torch.cuda.Stream()
    refs, hashes = [], []
    for pose in poses:
        pipe.gbuffer_frame, pipe.bdpt_frame = 11, 12
        with torch.cuda.stream(side):
            pipe.update_geometry(pose)
            pipe.render_frame()
        torch.cuda.synchronize()
        refs.append(pipe.output.clone())
        hashes.append(pipe.ctx.recs_hash())
    assert not torch.equal(refs[0], refs[1]) and hashes[0] != hashes[1]
    pipe.gbuffer_frame, pipe.bdpt_frame = 11, 12
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        pipe.update_geometry(pt)
        pipe.render_frame()
        graph.capture_end()
    torch.cuda.synchronize()
    for k, pose in enumerate(poses):
        pt.copy_(pose)
        pipe.output.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(pipe.output, refs[k]), k
        assert pipe.ctx.recs_hash() == hashes[k], k
    del graph
    pipe.close()
    scene.close()


def test_piece_prepare_conventions(pkg, monkeypatch):
    """(6) No scene, after an update, inside a capture: BDPT_E_STATE, and the context goes on as it was; bdpt_set_scene
    drops the mode."""
    import torch
    lib, a = pkg.load_library(), pkg.abi
    scene, _ = _scene(pkg, "atrium", monkeypatch)
    p1 = deform(positions_of(scene.desc))
    ctx = pkg.Context(0)
    assert lib.bdpt_prepare(ctx._h, a.PREPARE_REFIT_PIECES) == -2  # no scene
    ctx.set_scene(scene.desc)
    ctx.update_geometry(p1)
    plain_hash = ctx.recs_hash()
    assert lib.bdpt_prepare(ctx._h, a.PREPARE_REFIT_PIECES) == -2  # after an update
    assert lib.bdpt_prepare(ctx._h, a.PREPARE_REFIT_PIECES | a.PREPARE_REFIT) == -2
    ctx.update_geometry(p1)
    assert ctx.recs_hash() == plain_hash  # (it keeps refitting plainly)
    ctx.set_scene(scene.desc)
    ctx.prepare(refit_pieces=True)
    ctx.update_geometry(p1)
    tight_hash = ctx.recs_hash()
    assert tight_hash != plain_hash
    ctx.set_scene(scene.desc)  # drops the mode
    ctx.update_geometry(p1)
    assert ctx.recs_hash() == plain_hash
    ctx.close()
    # inside a capture (the context's last call is in it)
    pipe = pkg.FramePipeline(scene, 32, 24, max_depth=2)
    h = pipe.ctx._h
    gp = pipe.gbuffer_params()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        pipe.ctx.gbuffer_execute(gp, pipe.gb, pipe._stream_ptr())
        assert lib.bdpt_prepare(h, a.PREPARE_REFIT_PIECES) == -2
        graph.capture_end()
    torch.cuda.synchronize()
    del graph
    pipe.update_geometry(p1)
    torch.cuda.synchronize()
    assert pipe.ctx.recs_hash() == plain_hash  # (nothing was prepared)
    pipe.close()
    scene.close()


@pytest.mark.parametrize("anim", ["--sway", "--bend"])
def test_cpp_host_tight_refit_renders_the_plain_refits_image(pkg, tmp_path, anim):
    """host/bdpt_render --tight-refit (RenderingPipeline::setTightRefit before the first update): the same image as
    without, bit for bit, with two frames in flight (every slot's context prepared)."""
    import os
    import subprocess
    import __graft_entry__ as ge
    exe = os.path.join(ge.PKG_DIR, "host", "bdpt_render")
    assert os.path.exists(exe), "host/bdpt_render not built (run __graft_entry__.build())"
    W, H = 64, 36
    imgs = []
    for k, extra in enumerate(([], ["--tight-refit"])):
        raw = tmp_path / f"out{k}.f32"
        r = subprocess.run([exe, "--scene", "atrium", "--width", str(W), "--height", str(H), "--frames", "3", "--depth", "3", "--inflight", "2",
                            anim, "0.004", "--out", str(tmp_path / f"o{k}.pfm"), "--raw", str(raw)] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("references refitted by their pieces" in r.stdout) == bool(extra), r.stdout
        imgs.append(np.fromfile(raw, np.float32).reshape(H, W, 4))
    assert np.isfinite(imgs[0]).all() and imgs[0][..., :3].mean() > 0.0
    assert np.array_equal(imgs[0].view(np.uint32), imgs[1].view(np.uint32)), f"{(imgs[0] != imgs[1]).any(axis=-1).sum()} pixels differ"
