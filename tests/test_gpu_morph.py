"""GPU tests of morph targets: bdpt_set_morph / bdpt_update_morphed (csrc/deform.hip in front of the device refit).
Everything is compared bit for bit: the morphed (and skinned) streams with the numpy float32 restatement of
tests/morph_numpy.py, the refitted records with the host refit of the restated positions, frames with the oracle rendering
the description that holds the restated arrays and with a context given them through bdpt_update_geometry — as
tests/test_gpu_skinning.py does for bdpt_update_skinned."""
import ctypes as C

import numpy as np
import pytest

import morph_numpy as mn
import skin_numpy as sn
from test_gpu_configs import _assert_frame_equals_oracle
from test_gpu_refit import RAY_KEYS, Moved, _frame
from test_refit_cpu import HostTree, moved_desc

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _assert_streams(ctx, expected, label):
    got = ctx.read_morphed()
    for name, g, e in zip(("positions", "normals", "bitangents"), got, expected):
        assert (g is None) == (e is None), f"{label}: {name}"
        if e is not None:
            assert np.array_equal(mn.bits(g), mn.bits(e)), f"{label}: {(mn.bits(g) != mn.bits(e)).any(axis=1).sum()} {name} differ"


@pytest.fixture(scope="module")
def atrium(pkg):
    """Scene.atrium(4, 30000) — bitangents, a ragged last wave — with a 3-bone rig, base arrays that hold -0.0 components,
    and two poses; made once and left unchanged"""
    scene = pkg.Scene.atrium(4, 30000)
    d = scene.desc
    assert d.bitangents and d.numVertices % 64 != 0
    r = sn.scene_rig(d, 53, 3)
    for k in "PNB":
        r[k] = mn.with_negative_zeros(r[k], ord(k), share=0.01)
    r["poses"] = [sn.make_pose(s, 3, r["pivot"], r["extent"]) for s in (1, 2)]
    yield scene, r
    scene.close()


@pytest.mark.parametrize("skinned", [True, False], ids=["skin", "noskin"])
@pytest.mark.parametrize("num_targets", [1, 3, 1024])
def test_kernel_equals_the_restatement(pkg, atrium, num_targets, skinned):
    """Host weights, then device weights of another pose, the kernel alone with what the host update staged; then
    positions only, positions plus normals, and positions plus bitangents.  Before the first update read_morphed returns
    the base."""
    scene, r = atrium
    d = scene.desc
    nv = int(d.numVertices)
    tg = mn.make_targets(60 + num_targets, nv, num_targets, scale=0.01 * r["extent"])
    ctx = pkg.Context(0)
    ctx.set_scene(d)
    (b0, n0), (b1, n1) = r["poses"]
    w0, w1 = mn.make_weights(0, num_targets), mn.make_weights(1, num_targets)
    for streams in ("pnb", "p", "pn", "pb"):
        N = r["N"] if "n" in streams else None
        B = r["B"] if "b" in streams else None
        t = mn.only(tg, N is not None, B is not None)
        if skinned:
            ctx.set_skin(r["P"], r["W"], r["I"], 3, N, B)
            mn.set_morph(ctx, t)
            assert ctx.morphed_buffers() == ctx.skinned_buffers()
        else:
            mn.set_morph(ctx, t, r["P"], N, B)
        _assert_streams(ctx, (r["P"], N, B), f"{streams}: before the first update")
        kw = lambda bones, nbones: dict(rig=r, bones=bones, normal_bones=nbones) if skinned else {}
        pal = lambda bones, nbones, f=(lambda x: x): ((f(bones), f(nbones) if N is not None else None) if skinned else ())
        ctx.update_morphed(w0, *pal(b0, n0))
        first = mn.morph(t, w0, r["P"], N, B, **kw(b0, n0))
        _assert_streams(ctx, first, f"{streams}: host weights")
        assert not np.array_equal(first[0], r["P"])
        tw = _dev(w1)
        tp = pal(b1, n1, _dev)
        ctx.update_morphed(tw, *tp)
        _assert_streams(ctx, mn.morph(t, w1, r["P"], N, B, **kw(b1, n1)), f"{streams}: device weights")
        # every path of the kernel, forced (at this vertex count an update gathers the palettes from global memory; without
        # a skin there is one path): the kernel alone, with what the host update staged, writes the first pose over the second
        for path in (pkg.abi.MORPH_PATH_GLOBAL, pkg.abi.MORPH_PATH_LDS):
            ctx.test_morph_kernel(path)
            _assert_streams(ctx, first, f"{streams}: forced path {path}")
            ctx.update_morphed(tw, *tp)
    assert ctx.refit_info().numUpdates == 16
    ctx.close()


@pytest.fixture(scope="module")
def large_rig(pkg):
    """A soup of just over SKIN_LDS_MIN_VERTICES vertices, one rig over 64 bones and one set of targets for it, made once
    and left unchanged"""
    scene = pkg.Scene.soup(3, 349600, 0.05)
    r = sn.scene_rig(scene.desc, 9, 64)
    tg = mn.make_targets(17, int(scene.desc.numVertices), 3, sparse=5000, scale=0.002 * r["extent"])
    yield scene, r, tg
    scene.close()


@pytest.mark.parametrize("num_bones", [64, 65])
def test_large_skin_takes_the_lds_path_up_to_its_palette_limit(pkg, large_rig, num_bones):
    """The path rule is the skinning kernel's: at SKIN_LDS_MIN_VERTICES vertices or more an update stages palettes of up to
    SKIN_LDS_BONES bones in LDS (64) and gathers larger ones from global memory (65; the rig uses its first 64).
    1 048 800 vertices — the first size past the threshold that no workgroup of the LDS path (1024 vertices) ends on —
    device weights and bones, all three streams; then the other path forced."""
    scene, r, tg = large_rig
    d = scene.desc
    assert pkg.abi.SKIN_LDS_MIN_VERTICES <= d.numVertices < pkg.abi.SKIN_LDS_MIN_VERTICES + 1024 and d.bitangents and d.numVertices % 1024
    ctx = pkg.Context(0)
    ctx.set_scene(d)
    ctx.set_skin(r["P"], r["W"], r["I"], num_bones, r["N"], r["B"])
    mn.set_morph(ctx, tg)
    bones, nbones = sn.make_pose(6 + num_bones, num_bones, r["pivot"], r["extent"], angle=0.02, shift=0.002)
    w = mn.make_weights(0, 3)
    expected = mn.morph(tg, w, r["P"], r["N"], r["B"], rig=r, bones=bones, normal_bones=nbones)
    ctx.update_morphed(w, bones, nbones, keep_light_maps=True)
    _assert_streams(ctx, expected, "large skin, host inputs")
    ctx.update_morphed(_dev(mn.make_weights(1, 3)), _dev(bones), _dev(nbones), keep_light_maps=True)
    for path in (pkg.abi.MORPH_PATH_GLOBAL, pkg.abi.MORPH_PATH_LDS, pkg.abi.MORPH_PATH_AUTO):
        ctx.test_morph_kernel(path)
        _assert_streams(ctx, expected, f"large skin, path {path}")
        if path != pkg.abi.MORPH_PATH_AUTO:
            ctx.update_morphed(_dev(mn.make_weights(1, 3)), _dev(bones), _dev(nbones), keep_light_maps=True)
    ctx.close()


def test_cornell_one_wave_with_the_tall_block_morphed(pkg):
    """64 vertices, exactly one wave, no skin: only the tall block's 20 vertices have entries; the others come back as
    the base, and the records equal the host refit of the restated positions."""
    scene = pkg.Scene.cornell()
    d = scene.desc
    assert d.numVertices == 64
    r = sn.scene_rig(d, 3, 2)
    P, N = mn.with_negative_zeros(r["P"], 1, share=0.02), r["N"]
    tg = mn.make_targets(5, 64, 3, bitangents=False, sparse=9, candidates=np.arange(44, 64), scale=20.0)
    assert tg["vertex"].min() >= 44 and 64 - 1 in tg["vertex"] and 44 in tg["vertex"]
    ctx = pkg.Context(0)
    ctx.set_scene(d)
    mn.set_morph(ctx, tg, P, N)
    host = HostTree(pkg, d, -1.0, -1.0, 1)
    for w in (np.array([1.25, 0.5, -0.75], np.float32), np.array([-0.0, 2.0, 0.0], np.float32)):
        ctx.update_morphed(_dev(w))
        ep, en, _ = mn.morph(tg, w, P, N)
        _assert_streams(ctx, (ep, en, None), "cornell")
        assert np.array_equal(mn.bits(ep[:44]), mn.bits(P[:44])) and np.signbit(ep[0, 0])
        host.refit(ep)
        assert ctx.recs_hash() == host.hash()
    assert np.array_equal(mn.bits(ep), mn.bits(P))  # (the second weights: only the empty target's is not zero)
    host.close()
    ctx.close()
    scene.close()


def test_zero_weights_with_a_skin_are_update_skinned(pkg, atrium):
    """All weights zero (either sign): the streams and records update_skinned leaves for the same palettes on a second
    context.  update_skinned on the context with the morph ignores the morph."""
    scene, r = atrium
    d = scene.desc
    tg = mn.make_targets(8, int(d.numVertices), 3, scale=0.01 * r["extent"])
    a, b = pkg.Context(0), pkg.Context(0)
    for ctx in (a, b):
        ctx.set_scene(d)
        ctx.set_skin(r["P"], r["W"], r["I"], 3, r["N"], r["B"])
    mn.set_morph(a, tg)
    bones, nbones = r["poses"][0]
    a.update_morphed(np.array([0.0, -0.0, -0.0], np.float32), bones, nbones)
    b.update_skinned(bones, nbones)
    _assert_streams(a, b.read_skinned(), "zero weights")
    assert a.recs_hash() == b.recs_hash()
    a.update_morphed(_dev(mn.make_weights(0, 3)), _dev(bones), _dev(nbones))
    assert a.recs_hash() != b.recs_hash()
    a.update_skinned(_dev(bones), _dev(nbones))
    _assert_streams(a, b.read_skinned(), "update_skinned on a context with a morph")
    assert a.recs_hash() == b.recs_hash()
    a.close()
    b.close()


def _desc3(pkg, d, p, n, b):
    x = moved_desc(pkg, d, p)
    if n is not None:
        x.normals = n.ctypes.data_as(C.POINTER(C.c_float))
    if b is not None:
        x.bitangents = b.ctypes.data_as(C.POINTER(C.c_float))
    return x


@pytest.mark.parametrize("which", ["atrium", "courtyard"])
def test_update_morphed_is_update_geometry_of_the_restated_arrays(pkg, ob, which):
    """The normal-mapped atrium (with a skin) and the alpha-masked courtyard (without), 96x54, depth 4, weights A, B, A:
    records, refit_info and the frame equal those of a context given the restated arrays through update_geometry; the
    frame equals the oracle's on the description that holds them; A's records come back."""
    scene = pkg.Scene.atrium(4, 30000) if which == "atrium" else pkg.Scene.courtyard(1, 30000)
    d = scene.desc
    skinned = which == "atrium"
    nb = 12
    r = sn.scene_rig(d, 21, nb)
    P, N, B = r["P"], r["N"], r["B"]
    tg = mn.make_targets(31, int(d.numVertices), 5, bitangents=B is not None, sparse=2000, scale=0.004 * r["extent"], unit_scale=0.05)
    pipe = pkg.FramePipeline(scene, 96, 54, max_depth=4, mat_index=0)
    other = pkg.FramePipeline(scene, 96, 54, max_depth=4, mat_index=0)
    _frame(pipe)
    rest = pipe.output.cpu().numpy().copy()
    if skinned:
        pipe.set_skin(P, r["W"], r["I"], nb, N, B)
        mn.set_morph(pipe, tg)
    else:
        mn.set_morph(pipe, tg, P, N, B)
    bones, nbones = sn.make_pose(30, nb, r["pivot"], r["extent"], angle=0.03, shift=0.004)
    hashes = []
    for k, seed in enumerate((0, 1, 0)):
        w = mn.make_weights(seed, 5)
        if skinned:
            args = (_dev(w), _dev(bones), _dev(nbones)) if k == 1 else (w, bones, nbones)
            ep, en, eb = mn.morph(tg, w, P, N, B, rig=r, bones=bones, normal_bones=nbones)
        else:
            args = (_dev(w),) if k == 1 else (w,)
            ep, en, eb = mn.morph(tg, w, P, N, B)
        pipe.update_morphed(*args)
        other.update_geometry(ep, en, eb)
        hashes.append(pipe.ctx.recs_hash())
        assert hashes[-1] == other.ctx.recs_hash(), k
        ri, oi = pipe.ctx.refit_info(), other.ctx.refit_info()
        assert (ri.numUpdates, ri.sahCost, ri.sahCostBuilt) == (oi.numUpdates, oi.sahCost, oi.sahCostBuilt) and ri.numUpdates == k + 1
    assert hashes[0] == hashes[2] != hashes[1]
    for p_ in (pipe, other):
        p_.gbuffer_frame, p_.bdpt_frame = 0xdeadbeef, 0x1337
    gp, p = _frame(pipe)
    c, _ = _assert_frame_equals_oracle(pkg, ob, Moved(scene, _desc3(pkg, d, ep, en, eb)), pipe, gp, p, f"morphed {which}")
    img = pipe.output.cpu().numpy().copy()
    assert not np.array_equal(img.view(np.uint32), rest.view(np.uint32))
    _frame(other)
    o = other.ctx.counters().as_dict()
    ref = other.output.cpu().numpy()
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), f"{(img != ref).any(axis=-1).sum()} pixels differ"
    for key in RAY_KEYS:
        assert c[key] == o[key], (key, c[key], o[key])
    other.close()
    pipe.close()
    scene.close()


def test_morphed_update_refits_by_pieces(pkg, monkeypatch):
    """After prepare(refit_pieces=True): update_morphed == update_geometry of the restated positions on another prepared
    context."""
    from test_gpu_refit_pieces import _scene
    scene, budgets = _scene(pkg, "atrium", monkeypatch)
    d = scene.desc
    r = sn.scene_rig(d, 7, 5)
    tg = mn.make_targets(4, int(d.numVertices), 3, scale=0.005 * r["extent"])
    a, b = pkg.Context(0), pkg.Context(0)
    for ctx in (a, b):
        ctx.set_scene(d)
        ctx.prepare(refit_pieces=True)
    a.set_skin(r["P"], r["W"], r["I"], 5, r["N"], r["B"])
    mn.set_morph(a, tg)
    bones, nbones = sn.make_pose(11, 5, r["pivot"], r["extent"], angle=0.05, shift=0.005)
    w = mn.make_weights(0, 3)
    ep, en, eb = mn.morph(tg, w, r["P"], r["N"], r["B"], rig=r, bones=bones, normal_bones=nbones)
    a.update_morphed(_dev(w), _dev(bones), _dev(nbones))
    b.update_geometry(ep, en, eb)
    assert a.recs_hash() == b.recs_hash()
    plain = pkg.Context(0)
    plain.set_scene(d)
    plain.update_geometry(ep, en, eb)
    assert plain.recs_hash() != a.recs_hash()  # (the tree has pieces: the plain refit is another tree)
    for x in (plain, a, b):
        x.close()
    scene.close()


def test_area_lights_follow_a_morph(pkg, ob):
    """The Cornell AreaScene with the ceiling patch and the textured emitter moved by a morph target: the emitter table
    equals the oracle's and a fresh context's on the morphed description, and the BDPT_PARAM_AREA_LIGHTS frame equals
    the oracle's."""
    from area_scenes import AreaScene, bits
    from test_gpu_area_lights_oracle import _check_info, _frames_match
    cornell = pkg.Scene.cornell()
    scene = AreaScene(pkg, cornell, point_light=True, relit=True)
    nv = scene.P.shape[0]
    idx = np.unique(np.concatenate([scene.I[scene.M == mid].reshape(-1) for mid in (3, int(scene.M[-4]))])).astype(np.uint32)
    c = scene.P[idx].mean(axis=0)
    grow = ((scene.P[idx] - c) * np.float32(0.5) + np.array([25.0, -15.0, 10.0], np.float32)).astype(np.float32)
    tg = dict(ts=np.array([0, idx.size, idx.size], np.uint32), vertex=idx, dP=grow, dN=None, dB=None, num_vertices=nv, num_targets=2)
    w = np.array([0.75, 3.0], np.float32)
    pipe = pkg.FramePipeline(scene, 48, 40, max_depth=5, mat_index=1)
    before = _check_info(pkg, ob, pipe, scene).totalWeight  # (the table exists from here on: the update refreshes it)
    mn.set_morph(pipe, tg, scene.P)
    pipe.update_morphed(_dev(w))
    ep, _, _ = mn.morph(tg, w, scene.P)
    assert not np.array_equal(ep[idx], scene.P[idx])
    moved = AreaScene(pkg, cornell, point_light=True, relit=True, positions=ep)
    assert np.array_equal(mn.bits(moved.P), mn.bits(ep))
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


def test_previous_pose_channel_follows_a_morphed_update(pkg, atrium):
    """keep_pose, update_morphed, bdpt_gbuffer_execute_motion: the PrevWorldPosition channel (and WorldPosition) equal
    those of the same sequence done with update_geometry."""
    import torch
    scene, r = atrium
    d = scene.desc
    tg = mn.make_targets(9, int(d.numVertices), 3, scale=0.01 * r["extent"])
    W, H = 64, 36
    a = pkg.FramePipeline(scene, W, H, max_depth=3, motion=True)
    b = pkg.FramePipeline(scene, W, H, max_depth=3, motion=True)
    a.set_skin(r["P"], r["W"], r["I"], 3, r["N"], r["B"])
    mn.set_morph(a, tg)
    raw = lambda t: t.contiguous().view(torch.uint8).cpu().numpy()
    for k, (bones, nbones) in enumerate(r["poses"]):
        w = mn.make_weights(k, 3)
        ep, en, eb = mn.morph(tg, w, r["P"], r["N"], r["B"], rig=r, bones=bones, normal_bones=nbones)
        for pipe in (a, b):
            pipe.ctx.keep_pose(pipe._stream_ptr())
        a.update_morphed(_dev(w), _dev(bones), _dev(nbones))
        b.update_geometry(ep, en, eb)
        for pipe in (a, b):
            pipe.gbuffer_frame = 0xdeadbeef + k
            pipe.prev_position.fill_(7.0)
            pipe.ctx.gbuffer_execute_motion(pipe.gbuffer_params(), pipe.gb, C.c_void_p(pipe.prev_position.data_ptr()), pipe._stream_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(raw(a.prev_position), raw(b.prev_position)), k
        assert np.array_equal(raw(a.channels["WorldPosition"]), raw(b.channels["WorldPosition"])), k
        pos, prev = a.channels["WorldPosition"].float().cpu().numpy(), a.prev_position.cpu().numpy()
        hit = pos[..., 3] == 1
        assert hit.sum() > W * H // 2 and (pos[hit][:, :3] != prev[hit][:, :3]).any(axis=1).mean() > 0.5
    a.close()
    b.close()


def test_morphed_update_and_frame_captured_in_a_hip_graph(pkg):
    """After set_morph a captured (device-pointer update_morphed, G-buffer, execute) replays what its weight and bone
    tensors hold at the replay, each frame equal to the uncaptured one.  set_morph and host-pointer inputs are refused
    inside the capture (BDPT_E_STATE) without breaking it."""
    import torch
    scene = pkg.Scene.atrium(5, 12000)
    d = scene.desc
    nb = 8
    r = sn.scene_rig(d, 31, nb)
    tg = mn.make_targets(12, int(d.numVertices), 6, sparse=1500, scale=0.004 * r["extent"], unit_scale=0.05)
    poses = [sn.make_pose(s, nb, r["pivot"], r["extent"], angle=0.04, shift=0.005) for s in (41, 42)]
    weights = [mn.make_weights(s, 6) for s in (0, 1)]
    pipe = pkg.FramePipeline(scene, 160, 90, max_depth=5, mat_index=0)
    pipe.set_skin(r["P"], r["W"], r["I"], nb, r["N"], r["B"])
    mn.set_morph(pipe, tg)
    tw, tb, tn = _dev(weights[0]), _dev(poses[0][0]), _dev(poses[0][1])
    side = torch.cuda.Stream()

    def load(k, same_pose=False):
        tw.copy_(torch.from_numpy(weights[k]))
        tb.copy_(torch.from_numpy(poses[0 if same_pose else k][0]))
        tn.copy_(torch.from_numpy(poses[0 if same_pose else k][1]))
        torch.cuda.synchronize()

    refs = []
    for k, same_pose in ((0, False), (1, False), (1, True)):  # (the last: only the weight tensor differs from the first)
        load(k, same_pose)
        with torch.cuda.stream(side):
            pipe.gbuffer_frame, pipe.bdpt_frame = 0xdeadbeef, 0x1337
            pipe.update_morphed(tw, tb, tn)
            pipe.render_frame()
        torch.cuda.synchronize()
        refs.append(pipe.output.clone())
    assert not torch.equal(refs[0], refs[1]) and not torch.equal(refs[0], refs[2]) and not torch.equal(refs[1], refs[2])
    updates = pipe.ctx.refit_info().numUpdates
    lib = pkg.load_library()
    load(0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        pipe.gbuffer_frame, pipe.bdpt_frame = 0xdeadbeef, 0x1337
        graph.capture_begin()
        pipe.update_morphed(tw, tb, tn)
        with pytest.raises(pkg.BdptError, match=r"\(-2\)"):
            pipe.ctx.update_morphed(weights[0], poses[0][0], poses[0][1], pipe._stream_ptr())  # host pointers while capturing
        md = mn.morph_desc(pkg.abi, tg)
        assert lib.bdpt_set_morph(pipe.ctx._h, C.byref(md)) == -2  # (the context's last call is in the capture)
        pipe.render_frame()
        graph.capture_end()
    torch.cuda.synchronize()
    for ref, (k, same_pose) in ((0, (0, False)), (2, (1, True)), (1, (1, False)), (0, (0, False))):
        load(k, same_pose)
        pipe.output.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(pipe.output, refs[ref]), (ref, k, same_pose)
    _assert_streams(pipe.ctx, mn.morph(tg, weights[0], r["P"], r["N"], r["B"], rig=r, bones=poses[0][0], normal_bones=poses[0][1]), "after the replays")
    assert pipe.ctx.refit_info().numUpdates == updates + 1  # (the captured call counted once; the refused ones not at all)
    del graph
    pipe.close()
    scene.close()


def test_morph_error_conventions(pkg):
    """The codes of include/bdpt.h "Morph targets" that need a live context; a refused call leaves scene, skin and morph
    as they were; bdpt_set_skin and bdpt_set_scene drop the morph."""
    lib, a = pkg.load_library(), pkg.abi
    scene = pkg.Scene.cornell()
    d = scene.desc
    r = sn.scene_rig(d, 3, 4, static_share=0.3)
    P, N, B = r["P"], r["N"], r["B"]
    assert B is not None
    nv = P.shape[0]
    bones, nbones = sn.make_pose(4, 4, r["pivot"], r["extent"], angle=0.05)
    tg = mn.make_targets(2, nv, 3, sparse=9, scale=5.0)
    w = mn.make_weights(0, 3)
    pb, pn, pi = (C.c_void_p() for _ in range(3))
    buffers = lambda h: lib.bdpt_morphed_buffers(h, C.byref(pb), C.byref(pn), C.byref(pi))

    def upd(w_=w, bones_=None, nb_=None, nt=3, n=0, memory=0, flags=0, reserved=0):
        u = a.MorphUpdate()
        u.weights = None if w_ is None else w_.ctypes.data
        u.bones = None if bones_ is None else bones_.ctypes.data
        u.normalBones = None if nb_ is None else nb_.ctypes.data
        u.numTargets, u.numBones, u.memory, u.flags = nt, n, memory, flags
        u.reserved[1] = reserved
        return u

    update = lambda h, u: lib.bdpt_update_morphed(h, C.byref(u), None)
    # no scene
    ctx = pkg.Context(0)
    good = mn.morph_desc(a, tg, P, N, B)
    assert lib.bdpt_set_morph(ctx._h, C.byref(good)) == -2 and lib.bdpt_set_morph(ctx._h, None) == -2
    assert update(ctx._h, upd()) == -2 and buffers(ctx._h) == -2
    # a scene, no morph
    ctx.set_scene(d)
    h = ctx._h
    assert update(h, upd()) == -2 and buffers(h) == -2
    assert lib.bdpt_set_morph(h, None) == 0  # (dropping no morph is no error)
    # NULL arguments
    assert lib.bdpt_set_morph(None, C.byref(good)) == -1 and lib.bdpt_update_morphed(None, C.byref(upd()), None) == -1
    assert lib.bdpt_update_morphed(h, None, None) == -1 and lib.bdpt_morphed_buffers(h, None, C.byref(pn), C.byref(pi)) == -1
    # bdpt_set_morph on a context without a skin
    short = dict(tg, num_vertices=nv - 1)
    many = dict(tg, num_targets=1025)
    dP = tg["dP"].copy()
    dP[3, 0] = np.nan
    for x, code, label in ((mn.morph_desc(a, short, P, N, B), -1, "numVertices"), (mn.morph_desc(a, many, P, N, B), -5, "numTargets 1025"),
                           (mn.morph_desc(a, tg, None, None, None), -1, "no base"), (mn.morph_desc(a, tg, P, None, B), -1, "dNormals without normals"),
                           (mn.morph_desc(a, dict(tg, dP=dP), P, N, B), -1, "delta NaN")):
        assert lib.bdpt_set_morph(h, C.byref(x)) == code, label
    assert update(h, upd()) == -2  # (none of them left a morph behind)
    # the morph, and bdpt_update_morphed's checks; palettes given without a skin
    assert lib.bdpt_set_morph(h, C.byref(good)) == 0 and buffers(h) == 0 and pb.value and pn.value and pi.value
    ctx._morph_vertices = nv
    h0 = ctx.recs_hash()
    wbad = w.copy()
    wbad[1] = np.inf
    for u, code, label in ((upd(w_=None), -1, "weights"), (upd(nt=2), -1, "numTargets"), (upd(n=4), -1, "numBones"), (upd(memory=2), -1, "memory"),
                           (upd(flags=2), -1, "flags"), (upd(reserved=1), -1, "reserved"), (upd(w_=wbad), -1, "weight inf"),
                           (upd(bones_=bones, n=4), -1, "bones without a skin"), (upd(nb_=nbones), -1, "normalBones without a skin")):
        assert update(h, u) == code, label
    assert ctx.recs_hash() == h0 and ctx.refit_info().numUpdates == 0
    assert update(h, upd()) == 0
    h1 = ctx.recs_hash()
    assert h1 != h0 and ctx.refit_info().numUpdates == 1
    # update_geometry stays usable and leaves the morph alone
    ctx.update_geometry(P)
    assert ctx.recs_hash() != h1
    assert update(h, upd()) == 0 and ctx.recs_hash() == h1
    # a refused bdpt_set_morph leaves the morph in place
    assert lib.bdpt_set_morph(h, C.byref(mn.morph_desc(a, short, P, N, B))) == -1 and update(h, upd()) == 0
    # bdpt_set_skin drops the morph (a NULL desc too); with a skin the base must be the skin's
    ctx.set_skin(P, r["W"], r["I"], 4, N)
    assert update(h, upd(bones_=bones, nb_=nbones, n=4)) == -2 and buffers(h) == -2
    assert lib.bdpt_set_morph(h, C.byref(good)) == -1  # base pointers with a skin
    assert lib.bdpt_set_morph(h, C.byref(mn.morph_desc(a, tg))) == -1  # bitangent deltas, a skin without bitangents
    nob = mn.only(tg, bitangents=False)
    assert lib.bdpt_set_morph(h, C.byref(mn.morph_desc(a, nob))) == 0
    bbad = bones.copy()
    bbad[1, 5] = np.nan
    for u, code, label in ((upd(), -1, "palettes missing"), (upd(bones_=bones, n=4), -1, "normalBones missing"),
                           (upd(bones_=bones, nb_=nbones, n=3), -1, "numBones"), (upd(bones_=bbad, nb_=nbones, n=4), -1, "bone NaN")):
        assert update(h, u) == code, label
    assert update(h, upd(bones_=bones, nb_=nbones, n=4)) == 0
    ep, en, _ = mn.morph(nob, w, P, N, None, rig=r, bones=bones, normal_bones=nbones)
    _assert_streams(ctx, (ep, en, None), "with a skin")
    assert lib.bdpt_set_skin(h, None) == 0
    assert update(h, upd()) == -2 and buffers(h) == -2
    # bdpt_set_scene drops it; bitangents for a scene without any
    assert lib.bdpt_set_morph(h, C.byref(good)) == 0
    nobit = a.SceneDesc()
    C.pointer(nobit)[0] = d
    nobit.bitangents = None
    ctx.set_scene(nobit)
    assert update(h, upd()) == -2 and buffers(h) == -2
    assert lib.bdpt_set_morph(h, C.byref(good)) == -1
    assert lib.bdpt_set_morph(h, C.byref(mn.morph_desc(a, nob, P, N, B))) == -1
    assert lib.bdpt_set_morph(h, C.byref(mn.morph_desc(a, nob, P, N))) == 0
    ctx.close()
    scene.close()


def test_tiled_loop_with_morphed_updates_equals_one_in_flight(pkg, atrium):
    """tiling.TileRenderer with two frames in flight and a morphed update before every frame accumulates the image of one
    frame in flight: update_morphed reaches both slots' contexts."""
    import torch
    scene, r = atrium
    d = scene.desc
    tg = mn.make_targets(14, int(d.numVertices), 3, scale=0.005 * r["extent"])
    W, H, D, frames = 96, 54, 4, 4
    ws = [_dev(np.array([0.25 * k, 1.0, 0.5 - k], np.float32)) for k in range(frames)]  # (alive until the end)
    tb, tn = _dev(r["poses"][0][0]), _dev(r["poses"][0][1])
    imgs = []
    for inflight in (1, 2):
        tiled = pkg.tiling.TileRenderer(scene, W, H, D, 0, 0, 1, 0, None, inflight)
        tiled.set_skin(r["P"], r["W"], r["I"], 3, r["N"], r["B"])
        tiled.set_morph(tg["ts"], tg["vertex"], tg["dP"], tg["dN"], tg["dB"])
        for k in range(frames):
            tiled.update_morphed(ws[k], tb, tn)
            tiled.state["accum"] = k
            tiled.step()
        torch.cuda.synchronize()
        imgs.append(tiled.last_frame.cpu().numpy().copy())
        if inflight == 2:
            hashes = {p.ctx.recs_hash() for p in tiled.pipes}
            assert len(tiled.pipes) == 2 and len(hashes) == 1
        tiled.close()
    assert np.isfinite(imgs[0]).all() and imgs[0][..., :3].mean() > 0.0
    assert np.array_equal(imgs[0].view(np.uint32), imgs[1].view(np.uint32)), f"{(imgs[0] != imgs[1]).any(axis=-1).sum()} pixels differ"
