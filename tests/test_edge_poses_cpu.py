"""Edge-case poses (tests/edge_poses.py) through the host refit hooks and the host trace hook: the animated path's
definition on the CPU (bvh.h bvhRefitNodeT, bvhQuantiseNode, bvhPadOf, bvhPieceBox, bvhTriGeom), which the device refit
matches bit for bit (tests/test_gpu_edge_poses.py).  For every pose of both scenes, refitted plainly and by pieces:

  * bdpt_host_bvh_refit_check passes and the refit's SAH cost is finite;
  * the tree answers as the linear scan over the posed triangles does in modes 0, 1 and 2 (prim and the bits of t, u, v;
    any hit: hit or miss), 20 480 rays per mode, and a tree built at the pose does too;
  * refitting back to the built positions gives the records a first refit to them gives;
  * the number of rays the scan hits is asserted exactly (HITS; zero where it cannot see the scene, edge_poses.BLIND), the
    refit is compared with the fresh build ray by ray (VS_FRESH), and a pose outside the stated range is refused.

A ray that differs from the scan passes only under the documented limit edge_poses.ILL_CONDITIONED (the scan's triangle,
in float64), and how many do is asserted per pose in EXCUSED.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import edge_poses as ep
from test_refit_cpu import HostTree

# Rays per (scene, pose) the documented limit excuses, as (plain, pieces, fresh build), each (mode 0, mode 1, mode 2).
# Everything not listed: none.  flat_centre / flat_zero: needles (of the atrium's 6000 flattened triangles about 1000 have
# no area; their determinant is rounding noise); flat_oblique: the "inside" family, rays inside the plane of the triangles
# they meet; some_collapsed: needles and slivers a few fp32 spacings high.  Of the 4832 closest hits on the flattened
# atrium that is 1.6 %, all in the family aimed at the triangles; with e1 = e2 = 0 stored for needles of a corner sine
# below 8 eps the flat poses measured none (multiples 0, 1, 4, 16, 64 of eps^2: 49, 35, 20, 6, 0 rays of an earlier
# batch), but the rule moves the records of the suite's own atrium (34 needles): include/bdpt.h "Animated scenes".
EXCUSED = {
    ("atrium_split", "flat_centre"): ((77, 61, 0), (77, 61, 0), (77, 61, 0)),
    ("atrium_split", "flat_zero"): ((77, 61, 0), (77, 61, 0), (77, 61, 0)),
    ("atrium_split", "flat_oblique"): ((828, 784, 263), (853, 800, 265), (868, 813, 264)),
    ("atrium_split", "some_collapsed"): ((7, 3, 0), (8, 4, 0), (11, 7, 0)),
    ("courtyard_clipped", "flat_centre"): ((31, 35, 0), (31, 35, 0), (31, 35, 0)),
    ("courtyard_clipped", "flat_zero"): ((31, 35, 0), (31, 35, 0), (31, 35, 0)),
    ("courtyard_clipped", "flat_oblique"): ((814, 768, 292), (814, 769, 292), (838, 785, 296)),
    ("courtyard_clipped", "some_collapsed"): ((1, 1, 0), (1, 1, 0), (2, 1, 0)),
}

# Rays the scan hits per (scene, pose), modes 0 / 1 / 2, of 20 480 (the batches are deterministic).  scale_1e13: the fp32
# ray / triangle test overflows for most pairs (edges of 1e14, products of three such): the scan keeps a quarter of its hits.
HITS = {
    ('atrium_split', 'built'): (11349, 11029, 11349),
    ('atrium_split', 'far_1e3'): (11368, 11048, 11368),
    ('atrium_split', 'far_3e4'): (11560, 11221, 11560),
    ('atrium_split', 'far_1e5'): (11478, 11156, 11478),
    ('atrium_split', 'scale_1e6'): (11349, 11029, 11349),
    ('atrium_split', 'scale_1e10'): (10360, 10040, 10360),
    ('atrium_split', 'scale_1e13'): (2925, 1959, 2925),
    ('atrium_split', 'flat_centre'): (4832, 4824, 4832),
    ('atrium_split', 'flat_zero'): (4832, 4824, 4832),
    ('atrium_split', 'flat_oblique'): (7251, 7056, 7251),
    ('atrium_split', 'mirror_x'): (11365, 7667, 11365),
    ('atrium_split', 'permuted'): (12295, 12257, 12295),
    ('atrium_split', 'neg_zero'): (11205, 10894, 11205),
    ('atrium_split', 'some_collapsed'): (10643, 9979, 10643),
    ('courtyard_clipped', 'built'): (11630, 11334, 11630),
    ('courtyard_clipped', 'far_1e3'): (11646, 11350, 11646),
    ('courtyard_clipped', 'far_3e4'): (11736, 11436, 11736),
    ('courtyard_clipped', 'far_1e5'): (11639, 11347, 11639),
    ('courtyard_clipped', 'scale_1e6'): (11630, 11334, 11630),
    ('courtyard_clipped', 'scale_1e10'): (10598, 10314, 10598),
    ('courtyard_clipped', 'scale_1e13'): (2686, 2341, 2686),
    ('courtyard_clipped', 'flat_centre'): (4841, 4836, 4841),
    ('courtyard_clipped', 'flat_zero'): (4841, 4836, 4841),
    ('courtyard_clipped', 'flat_oblique'): (7237, 7045, 7237),
    ('courtyard_clipped', 'mirror_x'): (11639, 7451, 11639),
    ('courtyard_clipped', 'permuted'): (11327, 11183, 11327),
    ('courtyard_clipped', 'neg_zero'): (11512, 11227, 11512),
    ('courtyard_clipped', 'some_collapsed'): (10859, 10360, 10859),
}
# Rays per (scene, pose) on which the refit's answer differs from the fresh build's, (plain, pieces), each per mode: all of
# them excused rays.
VS_FRESH = {
    ("atrium_split", "flat_centre"): ((1, 0, 0), (1, 0, 0)),
    ("atrium_split", "flat_zero"): ((1, 0, 0), (1, 0, 0)),
    ("atrium_split", "flat_oblique"): ((114, 116, 1), (100, 96, 1)),
    ("atrium_split", "some_collapsed"): ((4, 4, 0), (3, 3, 0)),
    ("courtyard_clipped", "flat_oblique"): ((94, 65, 6), (96, 63, 6)),
    ("courtyard_clipped", "some_collapsed"): ((1, 0, 0), (1, 0, 0)),
}
# (scan hits, of which the tree misses, of which it answers with a hit behind) among the 1344 signed-zero rays at x1e10: test_zero_direction_components_...
ZERO_DIR_LOST = (1209, 1206, 1)

_back = {}


def _records_at_built_pose(pkg, c, kind):
    """hash of the records of a first refit to the built positions"""
    key = (c.which, kind)
    if key not in _back:
        t = ep.tree(pkg, c.which, c.scene, c.budgets, kind)
        t.refit(c.p0)
        _back[key] = t.hash()
        t.close()
    return _back[key]


def _compare(c, t, what):
    """(rays per mode that differ from the scan and are excused, the answers); any other difference fails"""
    counts, answers = [], []
    for mode in ep.MODES:
        prim, tuv = t.trace(c.rays, mode, 0)
        bad = c.differs(mode, prim, tuv)
        ok = c.excused(mode, bad)
        left = bad & ~ok
        assert not left.any(), (f"{c.which} {c.name} {what} mode {mode}: rays that differ from the scan per family {c.tally(left)} "
                                f"(excused: {c.tally(ok)})")
        counts.append(int(ok.sum()))
        answers.append((prim, tuv))
    return tuple(counts), answers


def _differ(c, a, b):
    """rays per mode on which two trees' answers differ; each of them must be excused"""
    out = []
    for mode in ep.MODES:
        (pa, ta), (pb, tb) = a[mode], b[mode]
        off = ((pa >= 0) != (pb >= 0)) if mode == 2 else ((pa != pb) | (ta.view(np.uint32) != tb.view(np.uint32)).any(axis=1))
        assert not (off & ~c.excused(mode, off)).any(), (c.which, c.name, mode, c.tally(off))
        out.append(int(off.sum()))
    return tuple(out)


@pytest.mark.parametrize("name", ep.NAMES)
@pytest.mark.parametrize("which", ep.SCENES)
def test_pose_refitted_and_traced_like_the_scan(pkg, which, name):
    c = ep.case(pkg, which, name)
    lib = pkg.load_library()
    if c.pose.cls == "refused":
        info = pkg.abi.BvhInfo()
        assert np.isfinite(c.pose.pos).all()
        assert not lib.bdpt_host_bvh_create(C.byref(c.desc), 0, *c.budgets, C.byref(info))  # bdpt_set_scene's range check
        assert info.reserved >= 1 and info.numTriangles == 0  # (this refusal, not another: 1 + the first triangle out of range)
        return
    hits = [int((c.scan[m][0] >= 0).sum()) for m in ep.MODES]
    print(f"{which} {name}: the scan hits {hits} of {len(c.rays)} rays")
    if c.pose.cls == "blind":
        assert hits == [0, 0, 0]
    excused, sah, answers = [], {}, {}
    for kind in ep.KINDS:
        t = ep.tree(pkg, which, c.scene, c.budgets, kind)
        t.refit(c.pose.pos)
        t.check()
        ri = t.refit_info()
        assert math.isfinite(ri.sahCost) and ri.sahCost > 0 and ri.sahCostBuilt == t.info.sahCost
        sah[kind] = ri.sahCost
        n, answers[kind] = _compare(c, t, f"refit ({kind})")
        excused.append(n)
        t.refit(c.p0)
        assert t.hash() == _records_at_built_pose(pkg, c, kind), f"{kind}: the refit back to the built positions"
        t.close()
    # a piece box is intersected with its triangle's box, so the piece refit is never the looser tree
    assert sah["pieces"] <= sah["plain"], sah
    fresh = HostTree(pkg, c.desc, *c.budgets)
    n, answers["fresh"] = _compare(c, fresh, "fresh build")
    excused.append(n)
    fresh.close()
    print(f"{which} {name}: excused (plain, pieces, fresh) {tuple(excused)}")
    # the refit answers as a build at the pose does: directly, ray by ray (only excused rays may differ, and how many is pinned)
    vs_fresh = tuple(_differ(c, answers[kind], answers["fresh"]) for kind in ep.KINDS)
    print(f"{which} {name}: refit differs from the fresh build (plain, pieces) {vs_fresh}")
    assert tuple(excused) == EXCUSED.get((which, name), ((0, 0, 0),) * 3)
    assert vs_fresh == VS_FRESH.get((which, name), ((0, 0, 0),) * 2)
    if c.pose.cls == "hits":
        assert tuple(hits) == HITS.get((which, name)) and hits[0] > 0 and hits[2] == hits[0]


def test_zero_direction_components_beyond_the_stated_width(pkg):
    """The documented limit behind edge_poses.ZERO_DIR_MAX_EXTENT, asserted: at x1e10 (wider than 2^35) the signed-zero
    families, which the pose's own batch leaves out, do go wrong, and only one way: the tree misses rays the scan hits, it
    reports one behind the scan's, never one in front of it; below the width (x1e6) the same families are exact."""
    import edge_rays as er
    which = "atrium_split"
    counts = {}
    for name in ("scale_1e6", "scale_1e10"):
        c = ep.case(pkg, which, name)
        rs = ep._RayScene(c.pose.pos)
        assert (rs.ext <= ep.ZERO_DIR_MAX_EXTENT) == (name == "scale_1e6")
        rng = np.random.default_rng(3)
        rays = np.concatenate([er.axis_rays(rs, rng, 32), er.partly_zero_rays(rs, rng, 32)])
        t = ep.tree(pkg, which, c.scene, c.budgets, "pieces")
        t.refit(c.pose.pos)
        sp, st = t.trace(rays, 0, 1)
        tp, tt = t.trace(rays, 0, 0)
        t.close()
        lost = (sp >= 0) & (tp < 0)
        other = ~lost & ((sp != tp) | (st.view(np.uint32) != tt.view(np.uint32)).any(axis=1))
        # where the tree loses the scan's hit it may find one behind it, never one in front of it and never one of its own
        assert ((sp[other] >= 0) & (tp[other] >= 0) & (tt[other, 0] >= st[other, 0])).all(), name
        counts[name] = (int((sp >= 0).sum()), int(lost.sum()), int(other.sum()))
    print(f"zero-component rays (scan hits, lost by the tree, answered with a hit behind): {counts}")
    assert counts["scale_1e6"][1:] == (0, 0) and counts["scale_1e6"][0] > 500
    assert counts["scale_1e10"] == ZERO_DIR_LOST


def test_refit_arithmetic_is_defined_on_boxes_that_are_not_finite(tmp_path):
    """tests/sanitize/refit_edge_main.cpp, a program of its own built with UBSan and its float-cast-overflow check:
    bvhQuantiseNode, both bvhRefitNodeT instances, bvhPieceBox, bvhPadOf and bvhTriGeom on infinities, NaNs, the largest
    finite values and subnormals — the boxes an overflowing skin produces.  No conversion may be undefined (the device
    saturates where C++ says nothing), and a NaN plane quantises to 0, +inf to 255."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "refit_edge_main")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=undefined,float-cast-overflow",
                        "-fno-sanitize-recover=undefined,float-cast-overflow", "-I", os.path.join(root, "fyp-bidirectionalpathtracer_amd", "csrc"),
                        "-o", exe, os.path.join(root, "tests", "sanitize", "refit_edge_main.cpp"), "-lpthread"],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "refit edge run finished failures=0" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr, r.stderr[-4000:]


def test_host_skin_equals_the_restatement_on_edge_rigs(pkg):
    """edge_poses.skin_rigs on the atrium: bones with one, two and three zero scales, a mirror, a bone 1e5 extents away,
    weights (w, -w), subnormal weights, weights that overflow the blend, every vertex on the last bone of palettes of 1,
    64 and 65.  bdpt_host_skin equals the numpy fp32 restatement bit for bit (by class — zero, inf, NaN, sign — where
    the blend cancels or overflows), every rig reaches its pose, and the finite poses refit and check, plain and by pieces."""
    import skin_numpy as sn
    which = "atrium_split"
    scene, budgets = ep.fixture(pkg, which)
    p0 = ep.positions_of(scene.desc)
    lib = pkg.load_library()
    trees = {kind: ep.tree(pkg, which, scene, budgets, kind) for kind in ep.KINDS}
    seen = set()
    for rig in ep.skin_rigs(p0):
        rc, hp, _, _ = sn.host_skin(lib, pkg.abi, p0, rig.W, rig.I, rig.bones)
        assert rc == 0, rig.name
        with np.errstate(all="ignore"):
            want, _, _ = sn.skin(p0, rig.W, rig.I, rig.bones)
        if rig.kind == "bits":
            assert np.array_equal(sn.bits(hp), sn.bits(want)), (rig.name, int((sn.bits(hp) != sn.bits(want)).any(axis=1).sum()))
        else:
            assert np.array_equal(ep.value_class(hp), ep.value_class(want)), rig.name
        assert rig.reaches(hp), f"{rig.name}: the rig does not reach its pose"
        seen.add(rig.name)
        if rig.kind == "bits":  # an independent reading: float64 from the same fp32 inputs
            dev = ep.deviation(hp, ep.skin_f64(p0, rig.W, rig.I, rig.bones))
            print(f"skin {rig.name}: deviation from float64 {dev:.3e}")
            assert dev <= 4 * ep.RIG_DEVIATION["skin " + rig.name], (rig.name, dev)
        if np.isfinite(hp).all():
            for kind, t in trees.items():
                t.refit(hp)
                t.check()
                assert math.isfinite(t.refit_info().sahCost), (rig.name, kind)
    assert len(seen) == 11
    for t in trees.values():
        t.close()
    scene.close()


def test_host_morph_equals_the_restatement_on_edge_rigs(pkg):
    """edge_poses.morph_rigs on the atrium: 1, 3, 4, 5, 8 and 9 entries per vertex (around the batch of four), weights
    -0.0 and +0.0 on a base with -0.0 coordinates (skipped: the bits stay), a target that cancels the base exactly, one
    that flattens the mesh at weight 1, and a morph followed by a collapsing skin.  bdpt_host_morph equals the numpy fp32
    restatement bit for bit (by class where the base cancels), stays within four times the tabulated deviation of a
    float64 reading, every rig reaches its pose, and the poses refit and check, plain and by pieces."""
    import morph_numpy as mn
    import skin_numpy as sn
    which = "atrium_split"
    scene, budgets = ep.fixture(pkg, which)
    p0 = ep.positions_of(scene.desc)
    lib = pkg.load_library()
    trees = {kind: ep.tree(pkg, which, scene, budgets, kind) for kind in ep.KINDS}
    rigs = ep.morph_rigs(p0)
    assert [r.name for r in rigs] == ["entries", "zero_weights", "cancelling", "flatten", "entries_then_zero_z_skin"]
    for rig in rigs:
        sk = rig.skin
        rc, hp, _, _ = mn.host_morph(lib, pkg.abi, rig.tg, rig.weights, rig.base, rig=sk, bones=None if sk is None else sk["bones"])
        assert rc == 0, rig.name
        want, _, _ = mn.morph(rig.tg, rig.weights, rig.base, rig=sk, bones=None if sk is None else sk["bones"])
        if rig.kind == "bits":
            assert np.array_equal(sn.bits(hp), sn.bits(want)), (rig.name, int((sn.bits(hp) != sn.bits(want)).any(axis=1).sum()))
            w64 = ep.morph_f64(rig.base, rig.tg, rig.weights)
            if sk is not None:
                w64 = ep.skin_f64(w64, sk["W"], sk["I"], sk["bones"])
            dev = ep.deviation(hp, w64)
            print(f"morph {rig.name}: deviation from float64 {dev:.3e}")
            assert dev <= 4 * ep.RIG_DEVIATION["morph " + rig.name], (rig.name, dev)
        else:
            assert np.array_equal(ep.value_class(hp), ep.value_class(want)), rig.name
        assert rig.reaches(hp), f"{rig.name}: the rig does not reach its pose"
        for kind, t in trees.items():
            t.refit(hp)
            t.check()
            assert math.isfinite(t.refit_info().sahCost), (rig.name, kind)
    for t in trees.values():
        t.close()
    scene.close()
