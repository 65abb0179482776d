"""Host-side tests of the piece-tight refit (bvh.h "piece-tight refit", BDPT_PREPARE_REFIT_PIECES) through the host-only
hook bdpt_host_bvh_refit_pieces: a tree with split or clipped references, refitted by pieces, must answer every query
exactly as the linear scan over the moved triangles does, must be tighter than the plain refit of the same tree, must be
a pure function of the built tree and the positions, and must be the plain refit where the tree has no pieces.  No GPU:
the device refit is compared with this one bit for bit by tests/test_gpu_refit_pieces.py."""
import ctypes as C

import numpy as np
import pytest

from test_refit_cpu import HostTree, deform, positions_of, rays_in


class PieceTree(HostTree):
    def pieces(self):
        assert self.lib.bdpt_host_bvh_refit_pieces(self.h) == 0

    def trace_visits(self, rays, mode):
        """(prim, tuv, [node visits, triangle tests]) of the tree walk"""
        n = rays.shape[0]
        prim = np.zeros(n, np.int32)
        tuv = np.zeros((n, 3), np.float32)
        vis = (C.c_uint64 * 2)()
        assert self.lib.bdpt_host_bvh_trace(self.h, rays.ctypes.data, n, mode, 0, 0, prim.ctypes.data, tuv.ctypes.data, vis) == 0
        return prim, tuv, [int(vis[0]), int(vis[1])]


def fixture_with_pieces(pkg, which):
    if which == "atrium_split":
        return pkg.Scene.atrium(2, 6000), (1.0, 4.0, 1)
    return pkg.Scene.courtyard(2, 6000, 0.6), (-1.0, -1.0, 1)


def assert_has_pieces(t, scene, which):
    if which == "atrium_split":
        assert t.info.numReferences > scene.desc.numTriangles
    else:
        assert t.info.numReferences != scene.desc.numTriangles or t.info.numDropped > 0


@pytest.mark.parametrize("pose", ["built", "deformed", "deformed_far"])
@pytest.mark.parametrize("which", ["atrium_split", "courtyard_clipped"])
def test_piece_refit_answers_like_the_linear_scan(pkg, which, pose):
    """(1) 65 536 random rays per mode against the scan over the moved triangles, on trees that do have pieces."""
    scene, budgets = fixture_with_pieces(pkg, which)
    p0 = positions_of(scene.desc)
    p1 = {"built": p0, "deformed": deform(p0), "deformed_far": deform(p0, 9, 0.05)}[pose]
    t = PieceTree(pkg, scene.desc, *budgets)
    assert_has_pieces(t, scene, which)
    t.pieces()
    t.refit(p1)
    t.check()  # layout words as built; every reference's eight mapped corners inside every decoded ancestor box
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
    t.close()
    scene.close()


@pytest.mark.parametrize("which", ["atrium_split", "courtyard_clipped"])
def test_piece_refit_is_tighter_than_the_plain_refit(pkg, which):
    """(2) At the built pose the piece refit's SAH ratio lies below the midpoint between 1 and the plain refit's, and the
    closest-hit rays test fewer triangles."""
    scene, budgets = fixture_with_pieces(pkg, which)
    p0 = positions_of(scene.desc)
    plain = PieceTree(pkg, scene.desc, *budgets)
    tight = PieceTree(pkg, scene.desc, *budgets)
    assert_has_pieces(tight, scene, which)
    tight.pieces()
    plain.refit(p0)
    tight.refit(p0)
    rp, rt = plain.refit_info(), tight.refit_info()
    ratio_plain, ratio_tight = rp.sahCost / rp.sahCostBuilt, rt.sahCost / rt.sahCostBuilt
    rays = rays_in(np.random.default_rng(7), 65536, p0.min(axis=0), p0.max(axis=0))
    pp, pt, vp = plain.trace_visits(rays, 1)
    tp, tt, vt = tight.trace_visits(rays, 1)
    print(f"{which}: sahCost / sahCostBuilt plain {ratio_plain:.4f} pieces {ratio_tight:.4f}; "
          f"triangle tests of 65536 closest-hit rays plain {vp[1]} pieces {vt[1]}")
    assert (pp == tp).all() and (pt.view(np.uint32) == tt.view(np.uint32)).all()
    assert ratio_plain > 1.0
    assert ratio_tight < 0.5 * (1.0 + ratio_plain)
    assert vt[1] < vp[1]
    plain.close()
    tight.close()
    scene.close()


@pytest.mark.parametrize("which", ["atrium", "soup"])
def test_a_tree_without_pieces_gets_the_plain_refit(pkg, which):
    """(3) Split budgets 0, classify 0: every region is the whole triangle, so the records are the plain refit's."""
    scene = pkg.Scene.atrium(1, 20000) if which == "atrium" else pkg.Scene.soup(11, 8000, 0.4)
    p0 = positions_of(scene.desc)
    t = PieceTree(pkg, scene.desc, 0.0, 0.0, 0)
    built = t.hash()
    t.pieces()
    t.refit(p0)
    assert t.hash() == built
    t.check()
    p1 = deform(p0)
    plain = PieceTree(pkg, scene.desc, 0.0, 0.0, 0)
    plain.refit(p1)
    t.refit(p1)
    assert t.hash() == plain.hash() != built
    assert t.refit_info().sahCost == plain.refit_info().sahCost
    plain.close()
    t.close()
    scene.close()


def test_piece_refit_is_a_pure_function_of_the_built_tree_and_positions(pkg):
    """(4) refit(P1) then refit(P0) equals refit(P0) on a fresh handle, with pieces on both."""
    scene = pkg.Scene.courtyard(3, 5000, 0.5)
    p0 = positions_of(scene.desc)
    p1 = deform(p0, seed=9, amp=0.05)
    a = PieceTree(pkg, scene.desc, -1.0, -1.0, 1)
    b = PieceTree(pkg, scene.desc, -1.0, -1.0, 1)
    a.pieces()
    b.pieces()
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


def test_piece_hook_refuses_bad_arguments_and_a_refitted_tree(pkg):
    """(5)"""
    lib = pkg.load_library()
    assert lib.bdpt_host_bvh_refit_pieces(None) == -1  # BDPT_E_INVALID
    scene = pkg.Scene.cornell()
    t = PieceTree(pkg, scene.desc, 0.0, 0.0, 0)
    t.refit(positions_of(scene.desc))
    assert lib.bdpt_host_bvh_refit_pieces(t.h) == -2  # BDPT_E_STATE: the boxes as built are gone
    t.close()
    scene.close()


def test_the_prepare_flag_has_its_declared_value(pkg):
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bdpt.h")).read()
    m = re.search(r"#define BDPT_PREPARE_REFIT_PIECES (\d+)u", hdr)
    a = pkg.abi
    assert m and int(m.group(1)) == a.PREPARE_REFIT_PIECES == 128
    others = (a.PREPARE_PRIMARY | a.PREPARE_BMFR | a.PREPARE_REFIT | a.PREPARE_LIGHT_GROUPS | a.PREPARE_AREA_LIGHTS | a.PREPARE_LIGHT_GROUP_TABLE
              | a.PREPARE_MOTION)
    assert a.PREPARE_REFIT_PIECES & others == 0
