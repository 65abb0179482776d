"""GPU tests of skinning: bdpt_set_skin / bdpt_update_skinned (csrc/deform.hip in front of the device refit).  Everything is
compared bit for bit: the skinned streams with the numpy float32 restatement of tests/skin_numpy.py, the refitted records
with the host refit of the restated positions, frames with the oracle rendering the description that holds the restated
arrays — as tests/test_gpu_refit.py does for bdpt_update_geometry."""
import ctypes as C

import numpy as np
import pytest

import skin_numpy as sn
from test_gpu_configs import _assert_frame_equals_oracle
from test_gpu_refit import RAY_KEYS, Moved, _frame
from test_refit_cpu import HostTree, moved_desc, positions_of

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _set_skin(ctx, r, num_bones, normals=True, bitangents=True):
    ctx.set_skin(r["P"], r["W"], r["I"], num_bones, r["N"] if normals else None, r["B"] if bitangents and r["B"] is not None else None)


def _assert_streams(ctx, r, bones, nbones, label, normals=True, bitangents=True):
    N = r["N"] if normals else None
    B = r["B"] if bitangents else None
    ep, en, eb = sn.skin(r["P"], r["W"], r["I"], bones, nbones, N, B)
    gp, gn, gb = ctx.read_skinned()
    assert np.array_equal(sn.bits(gp), sn.bits(ep)), f"{label}: {(sn.bits(gp) != sn.bits(ep)).any(axis=1).sum()} positions differ"
    assert (gn is None) == (N is None) and (gb is None) == (B is None), label
    if N is not None:
        assert np.array_equal(sn.bits(gn), sn.bits(en)), f"{label}: normals"
    if B is not None:
        assert np.array_equal(sn.bits(gb), sn.bits(eb)), f"{label}: bitangents"
    return ep, en, eb


# both sides of the kernel's LDS threshold (palettes of up to SKIN_LDS_BONES bones are staged in LDS), the smallest and
# the largest palette
@pytest.mark.parametrize("num_bones", [1, 3, 64, 65, 1024])
def test_kernel_equals_the_restatement(pkg, num_bones):
    """Scene.atrium(4, 30000): bitangents and a ragged last wave.  Host bones, then device bones of another pose; then a
    skin without normals and bitangents, one without bitangents, and one without normals on both paths."""
    assert pkg.abi.SKIN_LDS_BONES == 64
    scene = pkg.Scene.atrium(4, 30000)
    d = scene.desc
    assert d.bitangents and d.numVertices % 64 != 0
    r = sn.scene_rig(d, 50 + num_bones, num_bones)
    ctx = pkg.Context(0)
    ctx.set_scene(d)
    _set_skin(ctx, r, num_bones)
    p, n, b = ctx.read_skinned()  # before the first update: the rest pose
    assert np.array_equal(sn.bits(p), sn.bits(r["P"])) and np.array_equal(sn.bits(n), sn.bits(r["N"])) and np.array_equal(sn.bits(b), sn.bits(r["B"]))
    bones, nbones = sn.make_pose(1, num_bones, r["pivot"], r["extent"])
    ctx.update_skinned(bones, nbones)
    ep, _, _ = _assert_streams(ctx, r, bones, nbones, "host bones")
    assert not np.array_equal(ep, r["P"])
    bones2, nbones2 = sn.make_pose(2, num_bones, r["pivot"], r["extent"])
    tb, tn = _dev(bones2), _dev(nbones2)
    ctx.update_skinned(tb, tn)
    _assert_streams(ctx, r, bones2, nbones2, "device bones")
    assert ctx.refit_info().numUpdates == 2
    # both paths of the kernel, forced (at this vertex count an update gathers from global memory): the kernel alone, with
    # the palette the host-bone update staged, writes the first pose over the second
    for path in (pkg.abi.SKIN_PATH_GLOBAL, pkg.abi.SKIN_PATH_LDS):
        ctx.test_skin_kernel(path)
        _assert_streams(ctx, r, bones, nbones, f"forced path {path}")
        ctx.update_skinned(tb, tn)
        _assert_streams(ctx, r, bones2, nbones2, "device bones again")
    _set_skin(ctx, r, num_bones, normals=False, bitangents=False)  # positions alone: normalBones may be left out
    ctx.update_skinned(tb)
    _assert_streams(ctx, r, bones2, None, "positions only", normals=False, bitangents=False)
    _set_skin(ctx, r, num_bones, normals=True, bitangents=False)
    ctx.update_skinned(bones, nbones)
    _assert_streams(ctx, r, bones, nbones, "no bitangents", bitangents=False)
    _set_skin(ctx, r, num_bones, normals=False, bitangents=True)
    ctx.update_skinned(bones)
    _assert_streams(ctx, r, bones, None, "no normals", normals=False)
    for path in (pkg.abi.SKIN_PATH_GLOBAL, pkg.abi.SKIN_PATH_LDS):
        ctx.update_skinned(tb)
        _assert_streams(ctx, r, bones2, None, "no normals, device bones", normals=False)
        ctx.test_skin_kernel(path)
        _assert_streams(ctx, r, bones, None, f"no normals, forced path {path}", normals=False)
    ctx.close()
    scene.close()


@pytest.fixture(scope="module")
def large_rig(pkg):
    """A soup of just over SKIN_LDS_MIN_VERTICES vertices and one rig over 64 bones for it, made once and left unchanged"""
    scene = pkg.Scene.soup(3, 349600, 0.05)
    r = sn.scene_rig(scene.desc, 9, 64)
    yield scene, r
    scene.close()


@pytest.mark.parametrize("num_bones", [64, 65])
def test_large_skin_takes_the_lds_path_up_to_its_palette_limit(pkg, large_rig, num_bones):
    """At SKIN_LDS_MIN_VERTICES vertices or more an update stages palettes of up to SKIN_LDS_BONES bones in LDS (64) and
    gathers larger ones from global memory (65; the rig uses its first 64): 1 048 800 vertices — the first size past the
    threshold that no workgroup of the LDS path (1024 vertices) ends on — device bones, all three streams."""
    scene, r = large_rig
    d = scene.desc
    assert pkg.abi.SKIN_LDS_MIN_VERTICES <= d.numVertices < pkg.abi.SKIN_LDS_MIN_VERTICES + 1024 and d.bitangents
    ctx = pkg.Context(0)
    ctx.set_scene(d)
    _set_skin(ctx, r, num_bones)
    bones, nbones = sn.make_pose(6 + num_bones, num_bones, r["pivot"], r["extent"], angle=0.02, shift=0.002)
    ctx.update_skinned(_dev(bones), _dev(nbones), keep_light_maps=True)
    _assert_streams(ctx, r, bones, nbones, "large skin")
    ctx.close()


def test_cornell_one_wave_with_the_tall_block_skinned(pkg):
    """64 vertices, exactly one wave: only the tall block's 20 vertices have weights; the others (ids beyond the palette)
    come back as they are."""
    scene = pkg.Scene.cornell()
    d = scene.desc
    assert d.numVertices == 64
    mask = np.arange(64) < 44
    r = sn.scene_rig(d, 3, 2, static_mask=mask)
    assert (r["I"][:44] == 0xFFFF).all() and not sn.is_static(r["W"])[44:].any()
    ctx = pkg.Context(0)
    ctx.set_scene(d)
    _set_skin(ctx, r, 2)
    bones, nbones = sn.make_pose(4, 2, r["P"][44:].mean(axis=0), r["extent"], angle=0.3)
    ctx.update_skinned(_dev(bones), _dev(nbones))
    ep, _, _ = _assert_streams(ctx, r, bones, nbones, "cornell", bitangents=r["B"] is not None)
    assert np.array_equal(sn.bits(ep[:44]), sn.bits(r["P"][:44])) and not np.array_equal(ep[44:], r["P"][44:])
    host = HostTree(pkg, d, -1.0, -1.0, 1)
    host.refit(ep)
    assert ctx.recs_hash() == host.hash()
    host.close()
    ctx.close()
    scene.close()


@pytest.mark.parametrize("which", ["atrium", "courtyard"])
def test_refit_after_skinning_equals_the_host_refit(pkg, which):
    """recs_hash after update_skinned == HostTree.refit of the restated positions; pose A, B, then A again gives A's."""
    scene = pkg.Scene.atrium(1, 30000) if which == "atrium" else pkg.Scene.courtyard(1, 30000)
    d = scene.desc
    nb = 24
    r = sn.scene_rig(d, 7, nb)
    ctx = pkg.Context(0)
    ctx.set_scene(d)
    host = HostTree(pkg, d, -1.0, -1.0, 1)
    assert ctx.recs_hash() == host.hash()
    _set_skin(ctx, r, nb)
    hashes = []
    for k, seed in enumerate((11, 12, 11)):
        bones, nbones = sn.make_pose(seed, nb, r["pivot"], r["extent"], angle=0.05, shift=0.005)
        if k == 1:
            ctx.update_skinned(_dev(bones), _dev(nbones))
        else:
            ctx.update_skinned(bones, nbones)
        ep, _, _ = sn.skin(r["P"], r["W"], r["I"], bones)
        host.refit(ep)
        hashes.append(ctx.recs_hash())
        assert hashes[-1] == host.hash(), k
    host.check()
    assert hashes[0] == hashes[2] != hashes[1]
    ri, hi = ctx.refit_info(), host.refit_info()
    assert ri.numUpdates == 3 and ri.sahCost == hi.sahCost
    host.close()
    ctx.close()
    scene.close()


def _desc3(pkg, d, p, n, b):
    x = moved_desc(pkg, d, p)
    x.normals = n.ctypes.data_as(C.POINTER(C.c_float))
    x.bitangents = b.ctypes.data_as(C.POINTER(C.c_float))
    return x


def test_skinned_frame_matches_oracle_and_update_geometry(pkg, ob):
    """The normal-mapped atrium, 96x54, depth 4: the frame after a skinned update equals the oracle's on the description
    with the three restated arrays and differs from the rest-pose frame; a second context given the restated arrays
    through update_geometry renders the same image with the same ray counters."""
    scene = pkg.Scene.atrium(4, 30000)
    d = scene.desc
    assert d.bitangents and any(d.materials[m].texNormal >= 0 for m in range(d.numMaterials))
    nb = 12
    r = sn.scene_rig(d, 21, nb)
    pipe = pkg.FramePipeline(scene, 96, 54, max_depth=4, mat_index=0)
    _frame(pipe)
    rest = pipe.output.cpu().numpy().copy()
    pipe.set_skin(r["P"], r["W"], r["I"], nb, r["N"], r["B"])
    for k, device in enumerate((True, False)):
        bones, nbones = sn.make_pose(30 + k, nb, r["pivot"], r["extent"], angle=0.03, shift=0.004)
        if device:
            pipe.update_skinned(_dev(bones), _dev(nbones))
        else:
            pipe.update_skinned(bones, nbones)
        pipe.gbuffer_frame, pipe.bdpt_frame = 0xdeadbeef, 0x1337  # (the rest-pose frame's counters: only the pose differs)
        gp, p = _frame(pipe)
        ep, en, eb = sn.skin(r["P"], r["W"], r["I"], bones, nbones, r["N"], r["B"])
        c, _ = _assert_frame_equals_oracle(pkg, ob, Moved(scene, _desc3(pkg, d, ep, en, eb)), pipe, gp, p, f"skinned, device={device}")
        img = pipe.output.cpu().numpy().copy()
        assert not np.array_equal(img.view(np.uint32), rest.view(np.uint32))
    other = pkg.FramePipeline(scene, 96, 54, max_depth=4, mat_index=0)
    other.update_geometry(ep, en, eb)
    other.gbuffer_frame, other.bdpt_frame = 0xdeadbeef, 0x1337
    _frame(other)
    o = other.ctx.counters().as_dict()
    ref = other.output.cpu().numpy()
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), f"{(img != ref).any(axis=-1).sum()} pixels differ"
    for key in RAY_KEYS:
        assert c[key] == o[key], (key, c[key], o[key])
    other.close()
    pipe.close()
    scene.close()


def test_area_lights_follow_a_bone(pkg, ob):
    """The Cornell AreaScene with the ceiling patch and the textured emitter scaled and moved by a bone: the emitter
    table's total weight equals a fresh context's on the skinned description (and the oracle's), and the
    BDPT_PARAM_AREA_LIGHTS frame equals the oracle's."""
    from area_scenes import AreaScene, bits
    from test_gpu_area_lights_oracle import _check_info, _frames_match
    cornell = pkg.Scene.cornell()
    scene = AreaScene(pkg, cornell, point_light=True, relit=True)
    nv = scene.P.shape[0]
    idx = np.unique(np.concatenate([scene.I[scene.M == mid].reshape(-1) for mid in (3, int(scene.M[-4]))]))
    W = np.zeros((nv, 4), np.float32)
    I = np.full((nv, 4), 0xFFFF, np.uint16)
    W[idx] = (0.25, 0.0, 0.75, 0.0)  # (the same bone twice: weights 0.25 + 0.75 of one matrix)
    I[idx] = (1, 0, 1, 0)
    c = scene.P[idx].mean(axis=0).astype(np.float64)
    A = np.diag([1.5, 1.0, 1.25])
    bone = np.eye(4)
    bone[:3, :3] = A
    bone[3, :3] = c - c @ A + np.array([25.0, -15.0, 10.0])
    bones = np.stack([np.eye(4), bone]).reshape(2, 16).astype(np.float32)
    pipe = pkg.FramePipeline(scene, 48, 40, max_depth=5, mat_index=1)
    before = _check_info(pkg, ob, pipe, scene).totalWeight  # (the table exists from here on: the update refreshes it)
    pipe.set_skin(scene.P, W, I, 2)
    pipe.update_skinned(_dev(bones))
    ep, _, _ = sn.skin(scene.P, W, I, bones)
    assert not np.array_equal(ep[idx], scene.P[idx])
    moved = AreaScene(pkg, cornell, point_light=True, relit=True, positions=ep)
    assert np.array_equal(sn.bits(moved.P), sn.bits(ep))
    g = _check_info(pkg, ob, pipe, moved)
    assert g.totalWeight != before
    fresh = pkg.Context(0)
    fresh.set_scene(moved.desc)
    f = fresh.area_light_info()
    assert f.numEmitters == g.numEmitters and bits([f.totalWeight]) == bits([g.totalWeight])
    fresh.close()
    _frames_match(pkg, ob, moved, pipe, 0, frames=1)
    pipe.close()
    cornell.close()


def test_skinned_update_and_frame_captured_in_a_hip_graph(pkg):
    """After set_skin a captured (device-bone update_skinned, G-buffer, execute) replays the pose its bone tensors hold at
    the replay: pose A's frame, then pose B's, each equal to the uncaptured frame.  set_skin and host bones are refused
    inside the capture (BDPT_E_STATE) without breaking it."""
    import torch
    scene = pkg.Scene.atrium(5, 12000)
    d = scene.desc
    nb = 8
    r = sn.scene_rig(d, 31, nb)
    poses = [sn.make_pose(s, nb, r["pivot"], r["extent"], angle=0.04, shift=0.005) for s in (41, 42)]
    pipe = pkg.FramePipeline(scene, 160, 90, max_depth=5, mat_index=0)
    pipe.set_skin(r["P"], r["W"], r["I"], nb, r["N"], r["B"])
    tb, tn = _dev(poses[0][0]), _dev(poses[0][1])
    side = torch.cuda.Stream()
    refs = []
    for bones, nbones in poses:
        tb.copy_(torch.from_numpy(bones))
        tn.copy_(torch.from_numpy(nbones))
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            pipe.gbuffer_frame, pipe.bdpt_frame = 0xdeadbeef, 0x1337
            pipe.update_skinned(tb, tn)
            pipe.render_frame()
        torch.cuda.synchronize()
        refs.append(pipe.output.clone())
    assert not torch.equal(refs[0], refs[1])
    updates = pipe.ctx.refit_info().numUpdates
    lib = pkg.load_library()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        pipe.gbuffer_frame, pipe.bdpt_frame = 0xdeadbeef, 0x1337
        graph.capture_begin()
        pipe.update_skinned(tb, tn)
        with pytest.raises(pkg.BdptError, match=r"\(-2\)"):
            pipe.ctx.update_skinned(poses[0][0], poses[0][1], pipe._stream_ptr())  # host bones while capturing
        sd = sn.skin_desc(pkg.abi, r["P"], r["W"], r["I"], nb)
        assert lib.bdpt_set_skin(pipe.ctx._h, C.byref(sd)) == -2  # (the context's last call is in the capture)
        pipe.render_frame()
        graph.capture_end()
    torch.cuda.synchronize()
    for k in (0, 1, 0):
        tb.copy_(torch.from_numpy(poses[k][0]))
        tn.copy_(torch.from_numpy(poses[k][1]))
        torch.cuda.synchronize()
        pipe.output.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(pipe.output, refs[k]), k
    ep, en, eb = sn.skin(r["P"], r["W"], r["I"], poses[0][0], poses[0][1], r["N"], r["B"])
    gp, gn, gb = pipe.ctx.read_skinned()
    assert np.array_equal(sn.bits(gp), sn.bits(ep)) and np.array_equal(sn.bits(gn), sn.bits(en)) and np.array_equal(sn.bits(gb), sn.bits(eb))
    assert pipe.ctx.refit_info().numUpdates == updates + 1  # (the captured call counted once; the refused ones not at all)
    del graph
    pipe.close()
    scene.close()


def test_skinning_error_conventions(pkg):
    """Every code of include/bdpt.h "Skinning"; a refused update leaves the next frame and numUpdates as they were;
    bdpt_set_scene drops the skin."""
    lib, a = pkg.load_library(), pkg.abi
    scene = pkg.Scene.cornell()
    d = scene.desc
    r = sn.scene_rig(d, 3, 4, static_share=0.3)
    P, W, I, N, B = r["P"], r["W"], r["I"], r["N"], r["B"]
    bones, nbones = sn.make_pose(4, 4, r["pivot"], r["extent"], angle=0.05)
    pb, pn, pi = (C.c_void_p() for _ in range(3))

    def upd(bones_=bones, nb_=nbones, n=4, memory=0, flags=0, reserved=0):
        u = a.SkinUpdate()
        u.bones = None if bones_ is None else bones_.ctypes.data
        u.normalBones = None if nb_ is None else nb_.ctypes.data
        u.numBones, u.memory, u.flags, u.reserved = n, memory, flags, reserved
        return u

    # no scene
    ctx = pkg.Context(0)
    good = sn.skin_desc(a, P, W, I, 4, N, B)
    assert lib.bdpt_set_skin(ctx._h, C.byref(good)) == -2
    assert lib.bdpt_update_skinned(ctx._h, C.byref(upd()), None) == -2
    assert lib.bdpt_skinned_buffers(ctx._h, C.byref(pb), C.byref(pn), C.byref(pi)) == -2
    # a scene, no skin
    ctx.set_scene(d)
    assert lib.bdpt_update_skinned(ctx._h, C.byref(upd()), None) == -2
    assert lib.bdpt_skinned_buffers(ctx._h, C.byref(pb), C.byref(pn), C.byref(pi)) == -2
    assert lib.bdpt_set_skin(ctx._h, None) == 0  # (dropping no skin is no error)
    # NULL arguments
    assert lib.bdpt_set_skin(None, C.byref(good)) == -1
    assert lib.bdpt_update_skinned(None, C.byref(upd()), None) == -1
    assert lib.bdpt_update_skinned(ctx._h, None, None) == -1
    assert lib.bdpt_skinned_buffers(ctx._h, None, C.byref(pn), C.byref(pi)) == -1
    # bdpt_set_skin
    moving = np.flatnonzero(~sn.is_static(W))
    cases = []
    x = sn.skin_desc(a, P[:-1], W[:-1], I[:-1], 4)
    cases.append((x, -1, "numVertices"))
    x = sn.skin_desc(a, P, W, I, 0)
    cases.append((x, -1, "numBones 0"))
    x = sn.skin_desc(a, P, W, I, 1025)
    cases.append((x, -5, "numBones 1025"))
    x = sn.skin_desc(a, P, W, I, 4)
    x.reserved[0] = 1
    cases.append((x, -1, "reserved"))
    for f in ("positions", "boneWeights", "boneIds"):
        x = sn.skin_desc(a, P, W, I, 4)
        setattr(x, f, None)
        cases.append((x, -1, f))
    P2 = P.copy()
    P2[7, 2] = np.inf
    cases.append((sn.skin_desc(a, P2, W, I, 4), -1, "rest position"))
    I2 = I.copy()
    I2[moving[0], 1] = 4
    cases.append((sn.skin_desc(a, P, W, I2, 4), -1, "id"))
    for x, code, label in cases:
        assert lib.bdpt_set_skin(ctx._h, C.byref(x)) == code, label
    assert lib.bdpt_update_skinned(ctx._h, C.byref(upd()), None) == -2  # (none of them left a skin behind)
    ctx.close()
    # bitangents for a scene without any
    nobit = a.SceneDesc()
    C.pointer(nobit)[0] = d
    nobit.bitangents = None
    pipe = pkg.FramePipeline(Moved(scene, nobit), 64, 64, max_depth=3, mat_index=0)
    h = pipe.ctx._h
    assert lib.bdpt_set_skin(h, C.byref(sn.skin_desc(a, P, W, I, 4, N, P))) == -1
    pipe.set_skin(P, W, I, 4, N)
    gp, p = _frame(pipe)
    before = pipe.output.cpu().numpy().copy()
    # bdpt_update_skinned
    badb = bones.copy()
    badb[2, 13] = np.nan
    badn = nbones.copy()
    badn[0, 0] = -np.inf
    for u, code, label in ((upd(bones_=None), -1, "bones"), (upd(nb_=None), -1, "normalBones"), (upd(n=3), -1, "numBones"),
                           (upd(n=0), -1, "numBones 0"), (upd(memory=2), -1, "memory"), (upd(flags=2), -1, "flags"),
                           (upd(reserved=1), -1, "reserved"), (upd(bones_=badb), -1, "bone NaN"), (upd(nb_=badn), -1, "normal bone inf")):
        assert lib.bdpt_update_skinned(h, C.byref(u), None) == code, label
    with pytest.raises(pkg.BdptError):
        pipe.update_skinned(badb, nbones)
    pipe.gbuffer_frame -= 1
    pipe.bdpt_frame -= 1
    _frame(pipe)
    after = pipe.output.cpu().numpy()
    assert np.array_equal(after.view(np.uint32), before.view(np.uint32))
    assert pipe.ctx.refit_info().numUpdates == 0
    # update_geometry on a skinned context overwrites the pose and leaves the rest pose alone
    pipe.update_skinned(bones, nbones)
    h1 = pipe.ctx.recs_hash()
    pipe.update_geometry(P)
    assert pipe.ctx.recs_hash() != h1
    pipe.update_skinned(bones, nbones)
    assert pipe.ctx.recs_hash() == h1
    assert lib.bdpt_skinned_buffers(h, C.byref(pb), C.byref(pn), C.byref(pi)) == 0 and pb.value and pn.value and not pi.value
    # a new scene drops the skin
    pipe.ctx.set_scene(nobit)
    assert lib.bdpt_update_skinned(h, C.byref(upd()), None) == -2
    assert lib.bdpt_skinned_buffers(h, C.byref(pb), C.byref(pn), C.byref(pi)) == -2
    pipe.close()
    scene.close()


def test_cpp_host_bend_frames_in_flight_equal_one_in_flight(pkg, tmp_path):
    """host/bdpt_render --bend (RenderingPipeline::setSkin, updateSkinned before every frame): three frames in flight give
    the image of one frame in flight, bit for bit, and it differs from the unbent image."""
    import os
    import subprocess
    import __graft_entry__ as ge
    exe = os.path.join(ge.PKG_DIR, "host", "bdpt_render")
    assert os.path.exists(exe), "host/bdpt_render not built (run __graft_entry__.build())"
    W, H = 128, 72
    imgs = []
    for n, bend in ((1, "0.05"), (3, "0.05"), (1, None)):
        raw = tmp_path / f"out{n}{bend}.f32"
        cmd = [exe, "--scene", "atrium", "--width", str(W), "--height", str(H), "--frames", "4", "--depth", "4", "--inflight", str(n),
               "--out", str(tmp_path / f"o{n}{bend}.pfm"), "--raw", str(raw)]
        if bend:
            cmd += ["--bend", bend]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout + res.stderr
        imgs.append(np.fromfile(raw, np.float32).reshape(H, W, 4))
    assert np.isfinite(imgs[0]).all() and imgs[0][..., :3].mean() > 0.0
    assert np.array_equal(imgs[0].view(np.uint32), imgs[1].view(np.uint32)), f"{(imgs[0] != imgs[1]).any(axis=-1).sum()} pixels differ"
    assert not np.array_equal(imgs[0].view(np.uint32), imgs[2].view(np.uint32))
