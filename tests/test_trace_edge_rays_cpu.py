"""Edge-case rays (tests/edge_rays.py) through the host trace hook bdpt_host_bvh_*, whose tree walk states the slab
arithmetic of csrc/device_trace.hpp travInit / nodeStep: directions with +0.0 / -0.0 components, rays aimed exactly at
vertices and edges, hits at t == tmax and t == tmin, infinite tmax, negative tmin, direction lengths of 1e-20 to 1e30 and
the invalid rays, on a triangle soup at the origin and 64 away from it, a dyadic grid and the Cornell box.

Exact: the tree's answer is the linear scan's (closest hit: prim and the bits of t / u / v; any hit: hit or miss), in a
plain build and in the default split + clipped one, as built and after a refit; the oracle's scan and tree agree with it.
Independent: the scan's primitive is that of a float64 Moeller-Trumbore wherever float64 leaves no doubt.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import edge_rays as er
from test_refit_cpu import HostTree

BUILDS = {"plain": (0.0, 0.0, 0), "split_clipped": (-1.0, -1.0, 1)}


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name", er.SCENES)
def test_tree_answers_like_the_linear_scan(pkg, name, build):
    c = er.case(pkg, name)
    assert len(c.batch.rays) <= er.MAX_RAYS
    tree = HostTree(pkg, c.sc.desc, *BUILDS[build])
    for mode in er.MODES:
        er.assert_like_scan(c, mode, *tree.trace(c.batch.rays, mode, 0), f"tree ({build})")
    tree.close()
    # the batch is not vacuous: every family but the invalid rays has hits and misses of the closest-hit query
    prim = c.scan[0][0]
    for fam in c.batch.names:
        hit = prim[c.batch.of(fam)] >= 0
        if fam == "invalid":
            assert not hit.any()
        elif fam == "dyadic":
            assert hit.all()
        else:
            assert hit.any() and not hit.all(), fam


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name", er.SCENES)
def test_refitted_tree_answers_like_the_scan_of_the_moved_scene(pkg, name, build):
    """The tree built at the scene's place and refitted to the scene translated by (0.5, 0, 0), with the families made
    for the moved scene."""
    c = er.case(pkg, name, moved=True)
    tree = HostTree(pkg, c.built.desc, *BUILDS[build])
    tree.refit(c.sc.pos)
    tree.check()
    for mode in er.MODES:
        er.assert_like_scan(c, mode, *tree.trace(c.batch.rays, mode, 1), f"scan after the refit ({build})")
        er.assert_like_scan(c, mode, *tree.trace(c.batch.rays, mode, 0), f"refitted tree ({build})")
    tree.close()


@pytest.mark.parametrize("name", er.SCENES)
def test_oracle_scan_and_tree_agree_with_the_scan(pkg, ob, name):
    c = er.case(pkg, name)
    lib = ob.load_oracle(pkg.abi)
    osc = lib.oracle_scene_create(C.byref(c.sc.desc))
    n = len(c.batch.rays)
    for mode in er.MODES:
        for flags, what in ((ob.ORACLE_BRUTE_FORCE, "oracle scan"), (0, "oracle tree")):
            prim, tuv = np.zeros(n, np.int32), np.zeros((n, 3), np.float32)
            lib.oracle_trace(osc, c.batch.rays.ctypes.data, n, mode, flags, prim.ctypes.data, tuv.ctypes.data)
            er.assert_like_scan(c, mode, prim, tuv, what)
    lib.oracle_scene_destroy(osc)


@pytest.mark.parametrize("name", er.SCENES)
def test_scan_agrees_with_float64(pkg, name):
    """Guards the scan itself, which shares fp32 Moeller-Trumbore with the kernels: on the axis, partly-zero and wall
    families its closest primitive (and its any-hit answer) is float64's, for every ray float64 does not leave out; at
    most 2 % of a family may be left out.  (The grid's rays from vertex coordinates and to dyadic targets meet vertices
    and edges exactly, so the rule leaves all of them out: they are asserted exactly in test_grid_rays_to_dyadic_targets.)
    Measured shares left out: soup axis 0.26 %, partly_zero 0.17 %; soup64 0.39 %, 0.17 %; grid 0.00 %, 0.00 %;
    cornell axis 0.13 %, partly_zero 0.00 %, walls 0.20 %; no disagreement anywhere."""
    c = er.case(pkg, name)
    for fam in ("axis", "partly_zero", "walls"):
        if fam not in c.batch.names:
            continue
        sel = c.batch.of(fam)
        prim64, left = er.reference_f64(c.sc, c.batch.rays[sel])
        share = left.mean()
        wrong = int((c.scan[0][0][sel][~left] != prim64[~left]).sum())
        wrong_any = int(((c.scan[2][0][sel][~left] >= 0) != (prim64[~left] >= 0)).sum())
        print(f"{name} {fam}: {sel.sum()} rays, {100 * share:.2f} % left out, {wrong} closest and {wrong_any} any-hit disagreements")
        assert share <= er.F64_MAX_LEFT_OUT, (fam, share)
        assert wrong == 0 and wrong_any == 0, (fam, wrong, wrong_any)


def test_grid_rays_to_dyadic_targets(pkg):
    """Rays to every vertex, edge midpoint and diagonal midpoint of the grid, straight down and from four slanted
    offsets.  The arithmetic is exact in fp32, so: every ray hits, at t = 1.0 exactly, and the closest hit is the lowest
    index among the triangles that share the target (float64, exact here as well, names them)."""
    c = er.case(pkg, "grid")
    sel = c.batch.of("dyadic")
    rays = c.batch.rays[sel]
    assert len(rays) == 5 * 33 * 33
    want, _ = er.reference_f64(c.sc, rays)
    assert (want >= 0).all()
    tree = HostTree(pkg, c.sc.desc, *BUILDS["split_clipped"])
    for what, brute in (("scan", 1), ("tree", 0)):
        prim, tuv = tree.trace(rays, 0, brute)
        assert np.array_equal(prim, want), (what, int((prim != want).sum()))
        assert (tuv[:, 0] == np.float32(1.0)).all(), what
        assert (tree.trace(rays, 2, brute)[0] >= 0).all(), what
    tree.close()
