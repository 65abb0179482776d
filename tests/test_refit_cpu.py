"""Host-side tests of the refit behind bdpt_update_geometry (bvh.h "refit", csrc/bvh_build.cpp bvhRefitHost) through the
host-only hooks bdpt_host_bvh_refit / _refit_check / _recs_hash / _refit_info: the records of a tree refitted to moved
vertices must still answer every query exactly as the linear scan over the moved triangles does, keep their layout, and
be a pure function of the built topology and the current positions.  No GPU: the device refit (csrc/refit.hip) is
compared with this one bit for bit by tests/test_gpu_refit.py."""
import ctypes as C

import numpy as np
import pytest

import binding_fakes as fakes
from binding_fakes import RecordingLib, context_without_device


def positions_of(desc):
    return np.ctypeslib.as_array(desc.positions, shape=(desc.numVertices, 3)).copy()


def deform(p0, seed=3, amp=0.02):
    """A smooth deformation of every vertex plus a rigid move of a subset (the vertices on one side of the scene)."""
    rng = np.random.default_rng(seed)
    lo, hi = p0.min(axis=0), p0.max(axis=0)
    ext = float(np.max(hi - lo))
    k = rng.uniform(1.0, 3.0, 3) * (2 * np.pi / ext)
    ph = rng.uniform(0, 2 * np.pi, 3)
    p = p0.astype(np.float64)
    d = np.stack([np.sin(k[0] * p[:, 1] + ph[0]), np.sin(k[1] * p[:, 2] + ph[1]), np.sin(k[2] * p[:, 0] + ph[2])], axis=1)
    p = p + amp * ext * d
    side = p0[:, 0] > np.median(p0[:, 0])
    p[side] += np.array([0.03, -0.02, 0.05]) * ext
    return p.astype(np.float32)


def moved_desc(pkg, desc, positions):
    """A copy of `desc` whose positions are `positions` (kept alive by the caller)."""
    d = pkg.abi.SceneDesc()
    C.pointer(d)[0] = desc
    d.positions = positions.ctypes.data_as(C.POINTER(C.c_float))
    return d


class HostTree:
    def __init__(self, pkg, desc, budget, budget_alpha, classify):
        self.lib = pkg.load_library()
        self.pkg = pkg
        self.desc = desc
        self.info = pkg.abi.BvhInfo()
        self.h = self.lib.bdpt_host_bvh_create(C.byref(desc), 0, budget, budget_alpha, classify, C.byref(self.info))
        assert self.h

    def refit(self, positions):
        positions = np.ascontiguousarray(positions, np.float32)
        assert self.lib.bdpt_host_bvh_refit(self.h, positions.ctypes.data) == 0

    def check(self):
        msg = C.create_string_buffer(256)
        rc = self.lib.bdpt_host_bvh_refit_check(self.h, msg, 256)
        assert rc == 0, msg.value.decode()

    def hash(self):
        h = C.c_uint64()
        assert self.lib.bdpt_host_bvh_recs_hash(self.h, C.byref(h)) == 0
        return h.value

    def refit_info(self):
        r = self.pkg.abi.RefitInfo()
        assert self.lib.bdpt_host_bvh_refit_info(self.h, C.byref(r)) == 0
        return r

    def trace(self, rays, mode, brute):
        n = rays.shape[0]
        prim = np.zeros(n, np.int32)
        tuv = np.zeros((n, 3), np.float32)
        vis = (C.c_uint64 * 2)()
        assert self.lib.bdpt_host_bvh_trace(self.h, rays.ctypes.data, n, mode, brute, 0, prim.ctypes.data, tuv.ctypes.data, vis) == 0
        return prim, tuv

    def close(self):
        self.lib.bdpt_host_bvh_destroy(self.h)


def rays_in(rng, n, lo, hi, tmax=None):
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3] = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    r[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    r[:, 6] = 1e-4
    r[:, 7] = 1e38 if tmax is None else rng.uniform(0.1, tmax, n)
    return r


@pytest.mark.parametrize("which", ["atrium", "soup"])
def test_refit_to_the_built_positions_gives_the_built_records(pkg, which):
    """Split budgets 0, classify 0: every reference is its whole triangle, so refitting to the same positions must
    reproduce the records the builder packed, bit for bit, and the SAH cost it reported."""
    scene = pkg.Scene.atrium(1, 20000) if which == "atrium" else pkg.Scene.soup(11, 8000, 0.4)
    t = HostTree(pkg, scene.desc, 0.0, 0.0, 0)
    built = t.hash()
    t.refit(positions_of(scene.desc))
    assert t.hash() == built
    t.check()
    info = t.refit_info()
    assert info.sahCost == info.sahCostBuilt == t.info.sahCost
    t.close()
    scene.close()


@pytest.mark.parametrize("which", ["atrium_split", "courtyard_clipped"])
def test_refitted_tree_answers_like_the_linear_scan(pkg, which):
    """Moved vertices, a tree built with spatial splits (atrium) or with alpha-clipped and dropped foliage pieces
    (courtyard): 64 k random rays per mode, the refitted tree against the scan over the moved triangles."""
    if which == "atrium_split":
        scene = pkg.Scene.atrium(2, 6000)
        budgets = (1.0, 4.0, 1)
    else:
        scene = pkg.Scene.courtyard(2, 6000, 0.6)
        budgets = (-1.0, -1.0, 1)
    p0 = positions_of(scene.desc)
    p1 = deform(p0)
    t = HostTree(pkg, scene.desc, *budgets)
    if which == "atrium_split":
        assert t.info.numReferences > scene.desc.numTriangles  # the tree does have split references
    else:
        assert t.info.numDropped > 0 or t.info.numReferences != scene.desc.numTriangles
    t.refit(p1)
    t.check()  # layout words, prim / flags / aux as built; every triangle inside every decoded ancestor box
    rng = np.random.default_rng(7)
    lo, hi = p1.min(axis=0), p1.max(axis=0)
    n = 65536
    hits = 0
    for mode in (0, 1, 2):
        rays = rays_in(rng, n, lo, hi, None if mode != 2 else float(np.max(hi - lo)) * 0.5)
        prim, tuv = t.trace(rays, mode, 0)
        bprim, btuv = t.trace(rays, mode, 1)
        if mode == 2:
            assert ((prim >= 0) == (bprim >= 0)).all()
        else:
            assert (prim == bprim).all()
            assert (tuv.view(np.uint32) == btuv.view(np.uint32)).all()
            hits += int((prim >= 0).sum())
    assert hits > n // 4, "the sample must actually hit the moved scene"
    r = t.refit_info()
    assert r.sahCostBuilt == t.info.sahCost and r.sahCost > 0
    t.close()
    scene.close()


def test_refit_is_a_pure_function_of_topology_and_positions(pkg):
    """refit(P1) then refit(P0) equals refit(P0) on a fresh build: nothing of an earlier update survives."""
    scene = pkg.Scene.courtyard(3, 5000, 0.5)
    p0 = positions_of(scene.desc)
    p1 = deform(p0, seed=9, amp=0.05)
    a = HostTree(pkg, scene.desc, -1.0, -1.0, 1)
    b = HostTree(pkg, scene.desc, -1.0, -1.0, 1)
    a.refit(p1)
    moved = a.hash()
    a.refit(p0)
    b.refit(p0)
    assert a.hash() == b.hash()
    assert moved != a.hash()
    b.refit(p1)
    assert b.hash() == moved
    a.check()
    a.close()
    b.close()
    scene.close()


def test_refit_hooks_refuse_bad_arguments(pkg):
    lib = pkg.load_library()
    assert lib.bdpt_host_bvh_refit(None, None) == -1
    h = C.c_uint64()
    assert lib.bdpt_host_bvh_recs_hash(None, C.byref(h)) == -1
    scene = pkg.Scene.cornell()
    t = HostTree(pkg, scene.desc, 0.0, 0.0, 0)
    msg = C.create_string_buffer(64)
    assert lib.bdpt_host_bvh_refit_check(t.h, msg, 64) == -1  # nothing refitted yet
    t.close()
    scene.close()


def test_new_entry_points_have_their_declared_layouts(pkg):
    assert C.sizeof(pkg.abi.GeometryUpdate) == 40
    assert C.sizeof(pkg.abi.RefitInfo) == 16
    assert pkg.abi.PREPARE_REFIT == 4 and pkg.abi.UPDATE_KEEP_LIGHT_MAPS == 1
    assert (pkg.abi.MEMORY_HOST, pkg.abi.MEMORY_DEVICE) == (0, 1)


def _context_without_device(pkg, device=0):
    """a Context whose library records what bdpt_update_geometry was handed"""
    return context_without_device(pkg, RecordingLib({"bdpt_update_geometry": lambda g, stream: (g.memory, g.positions, g.normals,
                                                                                                g.numVertices)}), device)


def test_update_geometry_never_hands_host_memory_to_the_device_path(pkg):
    """A CPU torch tensor is host memory: Context.update_geometry sends it down the host path (checked and copied by the
    library), never its address as a device pointer; mixed host / GPU inputs and bad shapes are refused before anything
    reaches the library."""
    import torch
    ctx = _context_without_device(pkg)
    p = np.arange(12, dtype=np.float32).reshape(4, 3)
    t = torch.from_numpy(p.copy())
    ctx.update_geometry(t, normals=torch.ones(4, 3))
    mem, pos, nrm, n = ctx._lib.calls[-1]
    assert mem == pkg.abi.MEMORY_HOST and n == 4 and pos is not None and nrm is not None
    ctx.update_geometry(p)
    assert ctx._lib.calls[-1][0] == pkg.abi.MEMORY_HOST
    calls = len(ctx._lib.calls)
    with pytest.raises(pkg.BdptError):
        ctx.update_geometry(p, normals=np.ones((3, 3), np.float32))  # normals of another vertex count
    with pytest.raises(pkg.BdptError):
        ctx.update_geometry(np.ones(10, np.float32))  # not numVertices x 3

    def FakeGpuTensor(index):  # four positions in GPU memory
        return fakes.FakeGpuTensor((4, 3), torch.float32, index, ptr=0x1000)

    with pytest.raises(pkg.BdptError):
        ctx.update_geometry(FakeGpuTensor(1))  # another GPU's memory
    with pytest.raises(pkg.BdptError):
        ctx.update_geometry(FakeGpuTensor(0), normals=torch.ones(4, 3))  # GPU positions, host normals
    assert len(ctx._lib.calls) == calls
    ctx.update_geometry(FakeGpuTensor(0))
    assert ctx._lib.calls[-1][0] == pkg.abi.MEMORY_DEVICE
