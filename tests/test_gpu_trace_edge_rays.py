"""GPU tests of the traversal kernels on the edge-case rays of tests/edge_rays.py (signed-zero direction components, rays
at vertices and edges, hits at t == tmax / t == tmin, infinite tmax, negative tmin, very short and very long directions,
invalid rays; soup at the origin and 64 away, dyadic grid, Cornell box), each scene's families in one batch mixed with
ordinary rays.  Every entry point must give the linear scan's answer: bdpt_trace_rays in its three modes and
bdpt_test_trace (bit for bit, also against the oracle's tree and scan), the persistent any-hit kernel through
bdpt_test_trace_shadow, and bdpt_trace_rays behind a device-side bdpt_update_geometry on one stream.  The scan itself is
checked against float64 by tests/test_trace_edge_rays_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import edge_rays as er
from test_gpu_trace_rays import MODES, _as_prim_tuv, _check_all, _gpu, _oracle, _assert_same, _to_bdpt, _trace_device

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", er.SCENES)
def test_trace_rays_and_test_trace_answer_like_the_scan(pkg, ob, gpu_ctx, name):
    c = er.case(pkg, name)
    gpu_ctx.set_scene(c.sc.desc)
    lib = ob.load_oracle(pkg.abi)
    osc = lib.oracle_scene_create(C.byref(c.sc.desc))
    rays = c.batch.rays
    for m, mode in enumerate(MODES):
        er.assert_like_scan(c, m, *gpu_ctx.test_trace(rays, m), "bdpt_test_trace")
        er.assert_like_scan(c, m, *_trace_device(gpu_ctx, rays, mode), "bdpt_trace_rays")
        prim = _check_all(gpu_ctx, lib, osc, rays, mode, len(rays))  # == oracle tree == oracle scan == bdpt_test_trace, bit for bit
        assert (prim[c.batch.of("invalid")] == -1).all()
    if name == "grid":  # exact arithmetic: every ray to a dyadic target hits, at t = 1
        prim, tuv = _trace_device(gpu_ctx, rays, "closest")
        sel = c.batch.of("dyadic")
        assert (prim[sel] >= 0).all() and (tuv[sel, 0] == np.float32(1.0)).all()
    lib.oracle_scene_destroy(osc)


@pytest.mark.parametrize("name", er.SCENES)
def test_any_hit_kernel_one_launch_per_tmin(pkg, gpu_ctx, name):
    """trace_shadow_kernel takes one tmin per launch: the batch's rays grouped by their tmin (the families' common value,
    0 and the negative one), and eight rays of the interval family whose tmin is their own first hit's t, one launch each."""
    c = er.case(pkg, name)
    gpu_ctx.set_scene(c.sc.desc)
    rays = c.batch.rays
    occluded = c.scan[2][0] >= 0
    values, counts = np.unique(rays[:, 6], return_counts=True)
    assert (counts > 1).sum() >= 3
    groups = [np.flatnonzero(rays[:, 6] == v) for v in values[counts > 1]]
    own = np.flatnonzero(c.batch.of("interval") & np.isin(rays[:, 6], values[counts == 1]))
    assert len(own) >= 8
    groups += [own[k:k + 1] for k in range(8)]
    seen = 0
    for g in groups:
        vis, _ = gpu_ctx.test_trace_shadow(rays[g])
        assert set(np.unique(vis)) <= {0, 1}
        bad = np.zeros(len(rays), bool)
        bad[g] = (vis == 0) != occluded[g]
        assert not bad.any(), (name, float(rays[g[0], 6]), c.batch.tally(bad))
        seen += len(g)
    assert seen > 0.9 * len(rays)


@pytest.mark.parametrize("name", er.SCENES)
def test_trace_rays_after_update_geometry_on_the_same_stream(pkg, ob, gpu_ctx, name):
    """The tree built at the scene's place, refitted on the device to the scene translated by (0.5, 0, 0), then traced on
    the same stream: the answers are the moved scene's scan."""
    import torch
    c = er.case(pkg, name, moved=True)
    gpu_ctx.set_scene(c.built.desc)
    lib = ob.load_oracle(pkg.abi)
    osc = lib.oracle_scene_create(C.byref(c.sc.desc))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        st = C.c_void_p(side.cuda_stream)
        pos = _gpu(c.sc.pos)
        dev_rays = _gpu(_to_bdpt(c.batch.rays))
        gpu_ctx.update_geometry(pos, stream=st)
        res = {mode: gpu_ctx.trace_rays(dev_rays, mode, stream=st) for mode in MODES}
    torch.cuda.synchronize()
    for m, mode in enumerate(MODES):
        prim, tuv = _as_prim_tuv(res[mode], mode)
        er.assert_like_scan(c, m, prim, tuv, "bdpt_trace_rays after bdpt_update_geometry")
        _assert_same(prim, tuv, *_oracle(lib, osc, c.batch.rays, mode), (mode, "moved, oracle tree"))
    lib.oracle_scene_destroy(osc)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 4099])
def test_mixed_batch_sizes(pkg, gpu_ctx, n):
    """The wave width and the refill threshold kRefillIdle, each +-1, one ray, and a ragged tail: n consecutive rays of
    the soup's mixed batch, starting at an axis ray with a -0.0 component that hits."""
    c = er.case(pkg, "soup")
    gpu_ctx.set_scene(c.sc.desc)
    rays = c.batch.rays
    start = int(np.flatnonzero(c.batch.of("axis") & np.signbit(rays[:, 3:6]).any(axis=1) & (rays[:, 3:6] == 0).any(axis=1)
                               & (c.scan[0][0] >= 0))[0])
    idx = (start + np.arange(n)) % len(rays)
    assert n < 17 or len(np.unique(c.batch.family[idx])) > 2
    for m, mode in enumerate(MODES):
        prim, tuv = _trace_device(gpu_ctx, rays[idx], mode)
        sp, st = c.scan[m]
        if m == 2:
            assert np.array_equal(prim >= 0, sp[idx] >= 0), (n, mode)
        else:
            assert np.array_equal(prim, sp[idx]), (n, mode, int((prim != sp[idx]).sum()))
            assert np.array_equal(tuv.view(np.uint32), st[idx].view(np.uint32)), (n, mode)
        assert prim[0] >= 0  # the -0.0 ray hits
