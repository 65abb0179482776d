"""GPU tests of animated scenes: bdpt_update_geometry (the acceleration structure refitted in place on the device,
csrc/refit.hip) and bdpt_set_lights.  Every image is compared bit for bit — with the oracle rendering the moved scene
description, and with a fresh context bdpt_set_scene'd with it — as tests/test_gpu_configs.py does for static scenes."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_configs import _assert_frame_equals_oracle
from test_refit_cpu import HostTree, deform, moved_desc, positions_of

pytestmark = pytest.mark.gpu

RAY_KEYS = ("raysPrimary", "raysEyeExtend", "raysLightExtend", "raysNee", "raysSplat", "raysConnect", "pixelsValid",
            "splatsLanded", "raysConnectLazy", "hintedNee", "hintedSplat")


class Moved:
    """What the oracle helpers and FramePipeline read of a scene: its description (moved) and its camera."""

    def __init__(self, scene, desc):
        self.scene, self.desc = scene, desc

    def camera(self, aspect):
        return self.scene.camera(aspect)


def _torch_positions(p):
    import torch
    return torch.from_numpy(np.ascontiguousarray(p, np.float32)).cuda()


def _cornell_moved(scene, dx=-40.0, dz=25.0):
    """The tall block (the last five quads, 20 vertices) moved rigidly."""
    p0 = positions_of(scene.desc)
    assert p0.shape[0] == 64
    p1 = p0.copy()
    p1[-20:, 0] += dx
    p1[-20:, 2] += dz
    return p1


def _frame(pipe):
    import torch
    gp, p = pipe.render_frame()
    torch.cuda.synchronize()
    return gp, p


@pytest.mark.parametrize("which", ["cornell", "atrium", "courtyard"])
def test_device_refit_equals_host_refit(pkg, which):
    """The records after the same update: the device refit == the host refit, bit for bit (device and host inputs);
    the SAH cost of bdpt_get_refit_info == the host's."""
    scene = {"cornell": lambda: pkg.Scene.cornell(), "atrium": lambda: pkg.Scene.atrium(1, 262144),
             "courtyard": lambda: pkg.Scene.courtyard(1, 262144)}[which]()
    p0 = positions_of(scene.desc)
    p1 = _cornell_moved(scene) if which == "cornell" else deform(p0)
    ctx = pkg.Context(0)
    ctx.set_scene(scene.desc)
    host = HostTree(pkg, scene.desc, -1.0, -1.0, 1)
    assert ctx.recs_hash() == host.hash()  # (the same tree to start from)
    info0 = ctx.refit_info()
    assert info0.numUpdates == 0 and info0.sahCost == info0.sahCostBuilt == ctx.bvh_info().sahCost
    ctx.update_geometry(_torch_positions(p1))
    host.refit(p1)
    assert ctx.recs_hash() == host.hash()
    host.check()
    ri, hi = ctx.refit_info(), host.refit_info()
    assert ri.numUpdates == 1 and ri.sahCost == hi.sahCost and ri.sahCostBuilt == hi.sahCostBuilt
    moved = ctx.recs_hash()
    ctx.update_geometry(p0)  # host path back ...
    host.refit(p0)
    assert ctx.recs_hash() == host.hash()
    ctx.update_geometry(p1)  # ... and forth: the device state of earlier updates does not matter
    assert ctx.recs_hash() == moved
    host.close()
    ctx.close()
    scene.close()


def test_cornell_moved_block_matches_oracle(pkg, ob):
    """The tall block moved rigidly between frames: G-buffer channels, splat words and the image of two frames match the
    oracle rendering the moved description."""
    import torch
    scene = pkg.Scene.cornell()
    p1 = _cornell_moved(scene)
    d1 = moved_desc(pkg, scene.desc, p1)
    mv = Moved(scene, d1)
    pipe = pkg.FramePipeline(scene, 64, 64, max_depth=3, mat_index=0)
    _frame(pipe)
    pipe.update_geometry(_torch_positions(p1))
    names = {"WorldPosition": "worldPosition", "WorldNormal": "worldNormal", "MaterialDiffuse": "materialDiffuse",
             "MaterialSpecRough": "materialSpecRough", "MaterialExtraParams": "materialExtra", "Emissive": "emissive"}
    hip = C.CDLL("libamdhip64.so")
    for frame in range(2):
        gp, p = pipe.render_frame(extra_flags=pkg.abi.PARAM_DEFER_RESOLVE)
        torch.cuda.synchronize()
        orc = ob.OracleRender(pkg.abi, d1, pipe.W, pipe.H)
        orc.gbuffer(pipe.cam, gp)
        for ch, on in names.items():
            g = pipe.channels[ch].float().cpu().numpy().reshape(-1, 4)
            assert np.array_equal(g.view(np.uint32), orc.chan[on].view(np.uint32)), (frame, ch)
        orc.bdpt(pipe.cam, p)
        ptr, n64 = pipe.ctx.splat_buffer()
        spl = torch.empty(n64, dtype=torch.int64, device=pipe.dev)
        hip.hipMemcpy(C.c_void_p(spl.data_ptr()), C.c_void_p(ptr), C.c_size_t(n64 * 8), 3)
        assert np.array_equal(spl.cpu().numpy().view(np.uint64).reshape(-1, 4), orc.splat), frame
        orc.close()
        pipe.ctx.resolve(C.c_void_p(ptr), 0, C.c_void_p(pipe.output.data_ptr()), pipe._stream_ptr())
        torch.cuda.synchronize()
        _assert_frame_equals_oracle(pkg, ob, mv, pipe, gp, p, f"cornell moved frame {frame}")
    pipe.close()
    scene.close()


@pytest.mark.parametrize("which", ["atrium", "courtyard"])
def test_deformed_scene_matches_oracle_and_a_rebuild(pkg, ob, which):
    """configs[2] (atrium 262 k, depth 8) and the courtyard (262 k with alpha-masked foliage, depth 16) after a
    deformation: the frame equals the oracle's on the moved description and a fresh context's (bdpt_set_scene of the
    moved description) — image and ray tallies, hinted queries included (the light maps were re-traced: closest hits do
    not depend on the tree).  With BDPT_UPDATE_KEEP_LIGHT_MAPS the image stays exact."""
    import torch
    if which == "atrium":
        scene, W, H, D = pkg.Scene.atrium(1, 262144), 192, 108, 8
    else:
        scene, W, H, D = pkg.Scene.courtyard(1, 262144), 96, 54, 16
    p0 = positions_of(scene.desc)
    p1 = deform(p0, seed=5, amp=0.01)
    p2 = deform(p0, seed=6, amp=0.01)
    d1, d2 = moved_desc(pkg, scene.desc, p1), moved_desc(pkg, scene.desc, p2)
    pipe = pkg.FramePipeline(scene, W, H, max_depth=D, mat_index=0)
    _frame(pipe)
    pipe.update_geometry(_torch_positions(p1))
    gp, p = _frame(pipe)
    c, _ = _assert_frame_equals_oracle(pkg, ob, Moved(scene, d1), pipe, gp, p, f"{which} deformed")
    img = pipe.output.cpu().numpy().copy()
    fresh = pkg.FramePipeline(Moved(scene, d1), W, H, max_depth=D, mat_index=0)
    fresh.gbuffer_frame, fresh.bdpt_frame = pipe.gbuffer_frame - 1, pipe.bdpt_frame - 1
    _frame(fresh)
    f = fresh.ctx.counters().as_dict()
    ref = fresh.output.cpu().numpy()
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), f"{(img != ref).any(axis=-1).sum()} pixels differ"
    for k in RAY_KEYS:
        assert c[k] == f[k], (k, c[k], f[k])
    assert c["hintedNee"] > 0
    fresh.close()
    pipe.update_geometry(_torch_positions(p2), keep_light_maps=True)
    gp, p = _frame(pipe)
    _assert_frame_equals_oracle(pkg, ob, Moved(scene, d2), pipe, gp, p, f"{which} deformed, stale light maps")
    info = pipe.ctx.refit_info()
    assert info.numUpdates == 2 and info.sahCost > 0
    pipe.close()
    scene.close()


def test_animation_sequence_matches_oracle_and_returns(pkg, ob):
    """Four updates, one per frame, each frame equal to the oracle's on that frame's positions; back at the original
    positions with the first frame's counters, the first frame's image comes back bit for bit."""
    scene = pkg.Scene.atrium(3, 30000)
    p0 = positions_of(scene.desc)
    pipe = pkg.FramePipeline(scene, 96, 54, max_depth=5, mat_index=0)
    _frame(pipe)
    first = pipe.output.cpu().numpy().copy()
    for k in range(4):
        pk = deform(p0, seed=20 + k, amp=0.004 * (k + 1))
        pipe.update_geometry(pk)
        gp, p = _frame(pipe)
        _assert_frame_equals_oracle(pkg, ob, Moved(scene, moved_desc(pkg, scene.desc, pk)), pipe, gp, p, f"animation frame {k}")
    pipe.update_geometry(_torch_positions(p0))
    pipe.gbuffer_frame, pipe.bdpt_frame = 0xdeadbeef, 0x1337
    _frame(pipe)
    img = pipe.output.cpu().numpy()
    assert np.array_equal(img.view(np.uint32), first.view(np.uint32))
    pipe.close()
    scene.close()


def test_set_lights_matches_oracle(pkg, ob):
    """Moved point lights (Cornell) and the atrium's lights (point and spot) moved: frames equal the oracle's with the
    moved lights; the light count must stay."""
    for name in ("cornell", "atrium"):
        scene = pkg.Scene.cornell() if name == "cornell" else pkg.Scene.atrium(2, 20000)
        n = scene.desc.numLights
        lights = [pkg.abi.Light() for _ in range(n)]
        for i in range(n):
            C.memmove(C.byref(lights[i]), C.byref(scene.desc.lights[i]), C.sizeof(pkg.abi.Light))
            lights[i].posW[0] += 30.0 if name == "cornell" else 0.4
            lights[i].posW[2] -= 20.0 if name == "cornell" else 0.3
        arr = (pkg.abi.Light * n)(*lights)
        d1 = pkg.abi.SceneDesc()
        C.pointer(d1)[0] = scene.desc
        d1.lights = C.cast(arr, C.POINTER(pkg.abi.Light))
        pipe = pkg.FramePipeline(scene, 64, 64, max_depth=4, mat_index=0)
        _frame(pipe)
        pipe.set_lights(lights)
        for frame in range(2):
            gp, p = _frame(pipe)
            c, _ = _assert_frame_equals_oracle(pkg, ob, Moved(scene, d1), pipe, gp, p, f"{name} lights frame {frame}")
        with pytest.raises(pkg.BdptError):
            pipe.ctx.set_lights(lights + [lights[0]])
        pipe.close()
        scene.close()


def test_tiled_loop_with_updates_equals_plain_loop(pkg):
    """tiling.TileRenderer (three frames in flight, three contexts) with an update before every frame accumulates the
    image of the plain one-context loop with the same updates."""
    import torch
    scene = pkg.Scene.atrium(2, 20000)
    p0 = positions_of(scene.desc)
    W, H, D, frames = 128, 72, 5, 5
    poses = [_torch_positions(deform(p0, seed=40 + k, amp=0.003 * k)) for k in range(frames)]  # (alive until the end)
    plain = pkg.FramePipeline(scene, W, H, max_depth=D, mat_index=0, accum_limit=1 << 30)
    for k in range(frames):
        plain.update_geometry(poses[k])
        plain.accum_count = k  # (the running mean over the whole sequence, as the tiled loop below keeps it)
        plain.render_frame(accumulate=True)
    torch.cuda.synchronize()
    ref = plain.last_frame.cpu().numpy().copy()
    plain.close()
    tiled = pkg.tiling.TileRenderer(scene, W, H, D, 0, 0, 1, 0, None, 3)
    for k in range(frames):
        tiled.update_geometry(poses[k])
        tiled.state["accum"] = k
        tiled.step()
    torch.cuda.synchronize()
    img = tiled.last_frame.cpu().numpy()
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), f"{(img != ref).any(axis=-1).sum()} pixels differ"
    tiled.close()
    scene.close()


def test_update_and_frame_captured_in_a_hip_graph(pkg):
    """bdpt_prepare(BDPT_PREPARE_REFIT) then a captured (device-pointer update, G-buffer, execute) replays bit-exact."""
    import torch
    scene = pkg.Scene.atrium(5, 12000)
    p0 = positions_of(scene.desc)
    p1 = _torch_positions(deform(p0, seed=8, amp=0.01))
    p0t = _torch_positions(p0)
    pipe = pkg.FramePipeline(scene, 160, 90, max_depth=5, mat_index=0)
    pipe.ctx.prepare(pkg.abi.PREPARE_REFIT)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        pipe.update_geometry(p1)
        pipe.render_frame()
    torch.cuda.synchronize()
    ref = pipe.output.clone()
    pipe.gbuffer_frame, pipe.bdpt_frame = 0xdeadbeef, 0x1337
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        pipe.update_geometry(p0t)  # (outside the capture: the replay must move the scene back itself)
        graph.capture_begin()
        pipe.update_geometry(p1)
        pipe.render_frame()
        graph.capture_end()
    torch.cuda.synchronize()
    for _ in range(2):
        pipe.output.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(pipe.output, ref)
    del graph
    pipe.close()
    scene.close()


def test_update_error_conventions(pkg):
    """No scene: BDPT_E_STATE.  Wrong vertex count, a scene without bitangents given some, a wrong light count:
    BDPT_E_INVALID.  Too many lights: BDPT_E_LIMIT.  A NaN host position: BDPT_E_INVALID, and the next frame is the
    previous one, bit for bit."""
    import torch
    lib = pkg.load_library()
    ctx = pkg.Context(0)
    scene = pkg.Scene.cornell()
    p0 = positions_of(scene.desc)
    u = pkg.abi.GeometryUpdate()
    u.positions, u.numVertices, u.memory = p0.ctypes.data, p0.shape[0], pkg.abi.MEMORY_HOST
    assert lib.bdpt_update_geometry(ctx._h, C.byref(u), None) == -2
    light = pkg.abi.Light()
    assert lib.bdpt_set_lights(ctx._h, C.byref(light), 1, None) == -2
    ri = pkg.abi.RefitInfo()
    assert lib.bdpt_get_refit_info(ctx._h, C.byref(ri)) == -2
    ctx.close()
    nobit = pkg.abi.SceneDesc()  # (the Cornell box's materials have no normal map: its bitangents can be left out)
    C.pointer(nobit)[0] = scene.desc
    nobit.bitangents = None
    pipe = pkg.FramePipeline(Moved(scene, nobit), 64, 64, max_depth=3, mat_index=0)
    lib_ctx = pipe.ctx._h
    bad = p0.copy()
    u.positions, u.numVertices = bad.ctypes.data, p0.shape[0] - 1
    assert lib.bdpt_update_geometry(lib_ctx, C.byref(u), None) == -1
    u.numVertices = p0.shape[0]
    u.bitangents = p0.ctypes.data  # a scene without bitangents
    assert lib.bdpt_update_geometry(lib_ctx, C.byref(u), None) == -1
    u.bitangents = None
    lights = (pkg.abi.Light * 17)()
    assert lib.bdpt_set_lights(lib_ctx, lights, 17, None) == -5
    assert lib.bdpt_set_lights(lib_ctx, lights, 2, None) == -1
    gp, p = _frame(pipe)
    before = pipe.output.cpu().numpy().copy()
    bad = _cornell_moved(scene)
    bad[5, 1] = np.nan
    with pytest.raises(pkg.BdptError):
        pipe.update_geometry(bad)
    pipe.gbuffer_frame -= 1
    pipe.bdpt_frame -= 1
    _frame(pipe)
    after = pipe.output.cpu().numpy()
    assert np.array_equal(after.view(np.uint32), before.view(np.uint32))
    assert pipe.ctx.refit_info().numUpdates == 0
    pipe.close()
    scene.close()


def test_cpp_host_frames_in_flight_with_updates_equal_one_in_flight(pkg, tmp_path):
    """host/bdpt_render --sway (RenderingPipeline::updateGeometry before every frame): three frames in flight give the
    image of one frame in flight, bit for bit."""
    import os
    import subprocess
    import __graft_entry__ as ge
    exe = os.path.join(ge.PKG_DIR, "host", "bdpt_render")
    assert os.path.exists(exe), "host/bdpt_render not built (run __graft_entry__.build())"
    W, H = 128, 72
    imgs = []
    for n in (1, 3):
        raw = tmp_path / f"out{n}.f32"
        r = subprocess.run([exe, "--scene", "atrium", "--width", str(W), "--height", str(H), "--frames", "5", "--depth", "4",
                            "--inflight", str(n), "--sway", "0.004", "--out", str(tmp_path / f"o{n}.pfm"), "--raw", str(raw)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        imgs.append(np.fromfile(raw, np.float32).reshape(H, W, 4))
    assert np.isfinite(imgs[0]).all() and imgs[0][..., :3].mean() > 0.0
    assert np.array_equal(imgs[0].view(np.uint32), imgs[1].view(np.uint32)), f"{(imgs[0] != imgs[1]).any(axis=-1).sum()} pixels differ"


def test_moved_normals_and_bitangents_match_oracle(pkg, ob):
    """Normals and bitangents travel with an update (shading records and the bitangent array): on the normal-mapped
    atrium, device and host inputs, each frame equals the oracle's on the description with all three arrays replaced,
    and differs from the oracle's with the old normals, and with the old bitangents (both are read)."""
    import torch
    from test_gpu_parity import _oracle_frame
    scene = pkg.Scene.atrium(4, 30000)
    d = scene.desc
    assert d.bitangents and any(d.materials[m].texNormal >= 0 for m in range(d.numMaterials))
    p0 = positions_of(d)
    n0 = np.ctypeslib.as_array(d.normals, shape=(d.numVertices, 3)).copy()
    b0 = np.ctypeslib.as_array(d.bitangents, shape=(d.numVertices, 3)).copy()
    rng = np.random.default_rng(12)

    def perturb(v):
        w = v + rng.normal(scale=0.25, size=v.shape).astype(np.float32)
        return (w / np.maximum(np.linalg.norm(w, axis=1, keepdims=True), 1e-6)).astype(np.float32)

    def desc(p, n, b):
        x = moved_desc(pkg, d, p)
        x.normals = n.ctypes.data_as(C.POINTER(C.c_float))
        x.bitangents = b.ctypes.data_as(C.POINTER(C.c_float))
        return x

    def oracle_image(dd, pipe, gp, p):
        orc, _ = _oracle_frame(pkg, ob, Moved(scene, dd), pipe, gp, p)
        orc.resolve()
        img = orc.image().copy()
        orc.close()
        return img

    pipe = pkg.FramePipeline(scene, 96, 54, max_depth=4, mat_index=0)
    _frame(pipe)
    for k, device in enumerate((True, False)):
        p1 = deform(p0, seed=30 + k, amp=0.003)
        n1, b1 = perturb(n0), perturb(b0)
        if device:
            pipe.update_geometry(_torch_positions(p1), _torch_positions(n1), _torch_positions(b1))
        else:
            pipe.update_geometry(p1, n1, b1)
        gp, p = _frame(pipe)
        _assert_frame_equals_oracle(pkg, ob, Moved(scene, desc(p1, n1, b1)), pipe, gp, p, f"moved normals, device={device}")
        img = pipe.output.cpu().numpy()
        for label, dd in (("old normals", desc(p1, n0, b1)), ("old bitangents", desc(p1, n1, b0))):
            ref = oracle_image(dd, pipe, gp, p)
            assert not np.array_equal(img.view(np.uint32), ref.view(np.uint32)), f"{label}: the frame does not depend on them"
    pipe.close()
    scene.close()
