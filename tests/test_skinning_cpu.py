"""Host-side tests of skinning (include/bdpt.h "Skinning"): bdpt_host_skin — the per-vertex function the device kernel
runs (csrc/skin.h), compiled for the CPU — against the numpy float32 restatement of tests/skin_numpy.py, bit for bit;
struct layouts; error codes; and the host / device path choice of Context.update_skinned.  No GPU: the kernel is compared
with the same restatement by tests/test_gpu_skinning.py."""
import ctypes as C

import numpy as np
import pytest

import skin_numpy as sn
import binding_fakes as fakes
from binding_fakes import RecordingLib, context_without_device


def _soup_rig(pkg, seed, num_triangles, num_bones, **kw):
    scene = pkg.Scene.soup(seed, num_triangles, 0.4)
    d = scene.desc
    r = sn.scene_rig(d, seed + 100, num_bones, **kw)
    # (a soup has no bitangents: random unit vectors stand in, and its normals are perturbed so that no stream equals another)
    rng = np.random.default_rng(seed)
    b = rng.normal(size=r["P"].shape)
    r["B"] = (b / np.linalg.norm(b, axis=1, keepdims=True)).astype(np.float32)
    scene.close()
    return r


def _assert_matches(lib, abi, r, bones, nbones, streams="pnb"):
    N = r["N"] if "n" in streams else None
    B = r["B"] if "b" in streams else None
    rc, op, on, ob = sn.host_skin(lib, abi, r["P"], r["W"], r["I"], bones, nbones if N is not None else None, N, B)
    assert rc == 0
    ep, en, eb = sn.skin(r["P"], r["W"], r["I"], bones, nbones, N, B)
    assert np.array_equal(sn.bits(op), sn.bits(ep)), f"{(sn.bits(op) != sn.bits(ep)).any(axis=1).sum()} positions differ"
    if N is not None:
        assert np.array_equal(sn.bits(on), sn.bits(en))
    if B is not None:
        assert np.array_equal(sn.bits(ob), sn.bits(eb))
    return op, on, ob


@pytest.mark.parametrize("num_bones", [1, 3, 1024])
def test_host_skin_equals_the_restatement(pkg, num_bones):
    """A soup of about 8 000 triangles (24 003 vertices: no multiple of 64), palettes of 1, 3 and 1024 bones, every
    combination of streams."""
    lib = pkg.load_library()
    r = _soup_rig(pkg, 5, 8001, num_bones)
    assert r["P"].shape[0] % 64 != 0
    bones, nbones = sn.make_pose(9, num_bones, r["pivot"], r["extent"])
    st = sn.is_static(r["W"])
    assert 0 < st.sum() < st.size
    for streams in ("p", "pb", "pn", "pnb"):
        op, on, ob = _assert_matches(lib, pkg.abi, r, bones, nbones, streams)
    assert not np.array_equal(op[~st], r["P"][~st]) and not np.array_equal(on[~st], r["N"][~st])


def test_static_vertices_come_back_unchanged(pkg):
    """All four weights zero, of either sign: rest values bit for bit (-0.0 coordinates and a NaN-free but denormal one
    included), ids beyond the palette neither checked nor read."""
    lib = pkg.load_library()
    r = _soup_rig(pkg, 6, 500, 3, static_share=0.5)
    st = sn.is_static(r["W"])
    assert (r["I"][st] == 0xFFFF).all() and st.sum() > 100
    r["P"][st, 0] = np.float32(-0.0)
    r["P"][np.flatnonzero(st)[:7], 1] = np.float32(1e-41)
    r["N"][st, 2] = np.float32(-0.0)
    bones, nbones = sn.make_pose(2, 3, r["pivot"], r["extent"])
    op, on, ob = _assert_matches(lib, pkg.abi, r, bones, nbones)
    for out, rest in ((op, r["P"]), (on, r["N"]), (ob, r["B"])):
        assert np.array_equal(sn.bits(out[st]), sn.bits(rest[st]))
    assert np.signbit(op[st, 0]).all()


def test_weights_are_not_renormalised(pkg):
    lib = pkg.load_library()
    r = _soup_rig(pkg, 7, 700, 5, normalised=False)
    s = r["W"].astype(np.float64).sum(axis=1)
    assert (np.abs(s[~sn.is_static(r["W"])] - 1.0) > 1e-3).any()
    bones, nbones = sn.make_pose(3, 5, r["pivot"], r["extent"])
    _assert_matches(lib, pkg.abi, r, bones, nbones)


def test_skin_structs_and_constants(pkg):
    a = pkg.abi
    assert C.sizeof(a.SkinDesc) == 56 and C.sizeof(a.SkinUpdate) == 32
    assert a.SkinDesc.positions.offset == 8 and a.SkinDesc.boneIds.offset == 40 and a.SkinDesc.reserved.offset == 48
    assert a.SkinUpdate.numBones.offset == 16 and a.SkinUpdate.reserved.offset == 28
    assert a.BDPT_MAX_BONES == 1024
    lib = pkg.load_library()
    for name in ("bdpt_set_skin", "bdpt_update_skinned", "bdpt_skinned_buffers", "bdpt_host_skin"):
        assert hasattr(lib, name) and name in a.PROTOTYPES


def test_host_skin_error_codes(pkg):
    lib, a = pkg.load_library(), pkg.abi
    r = _soup_rig(pkg, 8, 40, 4, static_share=0.3)
    P, W, I, N, B = r["P"], r["W"], r["I"], r["N"], r["B"]
    bones, nbones = sn.make_pose(4, 4, r["pivot"], r["extent"])
    out = np.zeros_like(P)
    ptr = lambda x: x.ctypes.data

    def call(d, bones_=bones, nb=nbones, op=out, on=out, ob=out):
        return lib.bdpt_host_skin(C.byref(d) if d is not None else None, None if bones_ is None else ptr(bones_),
                                  None if nb is None else ptr(nb), None if op is None else ptr(op),
                                  None if on is None else ptr(on), None if ob is None else ptr(ob))

    good = lambda: sn.skin_desc(a, P, W, I, 4, N, B)
    assert call(good()) == 0
    assert call(None) == -1 and call(good(), bones_=None) == -1 and call(good(), op=None) == -1
    assert call(good(), nb=None) == -1 and call(good(), on=None) == -1 and call(good(), ob=None) == -1
    assert call(sn.skin_desc(a, P, W, I, 4), nb=None, on=None, ob=None) == 0  # positions alone need none of them
    for field in ("positions", "boneWeights", "boneIds"):
        d = good()
        setattr(d, field, None)
        assert call(d) == -1, field
    d = good()
    d.numBones = 0
    assert call(d) == -1
    d = good()
    d.numBones = 1025
    assert call(d) == -5
    d = good()
    d.reserved[1] = 1
    assert call(d) == -1
    moving = np.flatnonzero(~sn.is_static(W))
    static = np.flatnonzero(sn.is_static(W))
    I2 = I.copy()
    I2[moving[0], 3] = 4  # == numBones on a vertex with a weight (even where that slot's weight is zero)
    assert call(sn.skin_desc(a, P, W, I2, 4, N, B)) == -1
    I3 = I.copy()
    I3[static] = 4000  # a static vertex: not checked
    assert call(sn.skin_desc(a, P, W, I3, 4, N, B)) == 0
    for bad in (np.nan, np.inf):
        P2 = P.copy()
        P2[static[0], 1] = bad  # a rest position, static or not
        assert call(sn.skin_desc(a, P2, W, I, 4, N, B)) == -1
        W2 = W.copy()
        W2[moving[1], 0] = bad
        assert call(sn.skin_desc(a, P, W2, I, 4, N, B)) == -1


def _context_without_device(pkg, device=0):
    """a Context whose library records what bdpt_update_skinned (.calls) and bdpt_set_skin (.skins) were handed"""
    lib = RecordingLib({"bdpt_update_skinned": lambda g, stream: (g.memory, g.bones, g.normalBones, g.numBones, g.flags)})
    lib.skins = []

    def set_skin(h, d):
        lib.skins.append(None if d is None else (d._obj.numVertices, d._obj.numBones, d._obj.normals, d._obj.bitangents))
        return 0

    lib.bdpt_set_skin = set_skin
    return context_without_device(pkg, lib, device)


def test_update_skinned_picks_the_host_or_the_device_path(pkg):
    """numpy arrays and CPU tensors go down the host path (checked and staged by the library), GPU tensors down the device
    path; mixed inputs, another GPU's memory and bad shapes are refused before anything reaches the library."""
    import torch
    ctx = _context_without_device(pkg)
    m = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (3, 1))
    ctx.update_skinned(m)
    assert ctx._lib.calls[-1] == (pkg.abi.MEMORY_HOST, m.ctypes.data, None, 3, 0)
    ctx.update_skinned(torch.from_numpy(m.copy()), normal_bones=torch.from_numpy(m.copy()), keep_light_maps=True)
    mem, b, nb, n, flags = ctx._lib.calls[-1]
    assert mem == pkg.abi.MEMORY_HOST and b and nb and n == 3 and flags == pkg.abi.UPDATE_KEEP_LIGHT_MAPS
    calls = len(ctx._lib.calls)
    with pytest.raises(pkg.BdptError):
        ctx.update_skinned(m, normal_bones=m[:2])  # palettes of two sizes
    with pytest.raises(pkg.BdptError):
        ctx.update_skinned(np.ones(20, np.float32))  # not numBones x 16

    def FakeGpuTensor(index, contiguous=True):  # a palette of three bones in GPU memory
        return fakes.FakeGpuTensor((3, 16), torch.float32, index, contiguous, ptr=0x2000)

    with pytest.raises(pkg.BdptError):
        ctx.update_skinned(FakeGpuTensor(1))  # another GPU's memory
    with pytest.raises(pkg.BdptError):
        ctx.update_skinned(FakeGpuTensor(0), normal_bones=m)  # GPU bones, host inverse transposes
    with pytest.raises(pkg.BdptError):
        ctx.update_skinned(FakeGpuTensor(0, contiguous=False))
    assert len(ctx._lib.calls) == calls
    ctx.update_skinned(FakeGpuTensor(0), normal_bones=FakeGpuTensor(0))
    assert ctx._lib.calls[-1] == (pkg.abi.MEMORY_DEVICE, 0x2000, 0x2000, 3, 0)


def test_set_skin_binding_checks_shapes(pkg):
    ctx = _context_without_device(pkg)
    P = np.zeros((5, 3), np.float32)
    W = np.zeros((5, 4), np.float32)
    I = np.zeros((5, 4), np.uint16)
    ctx.set_skin(P, W, I, 2, normals=P)
    nv, nb, nrm, bit = ctx._lib.skins[-1]
    assert (nv, nb) == (5, 2) and nrm and not bit
    with pytest.raises(pkg.BdptError):
        ctx.set_skin(P, W[:4], I, 2)
    with pytest.raises(pkg.BdptError):
        ctx.set_skin(P, W, I, 2, bitangents=P[:3])
    ctx.set_skin(None, None, None, 0)
    assert ctx._lib.skins[-1] is None
