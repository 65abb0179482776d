"""GPU tests of the animated path on the edge-case poses of tests/edge_poses.py: bdpt_update_geometry (csrc/refit.hip
k_refit_scene_box, k_refit_pad, k_refit_level, k_refit_level_pieces) and the traversal of the refitted tree by
bdpt_trace_rays.  One context per scene and refit kind, updated pose by pose: after every update the device's records and
SAH cost equal the host refit's bit for bit, and closest-hit and any-hit queries equal the host tree walk bit for bit
(but for the rays counted in DEVICE_OFF, under the documented limit edge_poses.ILL_CONDITIONED), which tests/test_edge_poses_cpu.py pins to
the linear scan.  A pose outside the stated range of positions is refused and
leaves the context as it was.  Each batch is the first 4096 rays of the pose's 20 480 (every family is in it; 1024 at the tiny scales)."""
import ctypes as C
import struct

import numpy as np
import pytest

import edge_poses as ep
from test_gpu_refit import _torch_positions
from test_gpu_trace_rays import MODES, _trace_device

pytestmark = pytest.mark.gpu

N_RAYS = 4096
N_RAYS_TINY = 1024  # the tiny scales: the host walk they are compared with computes in subnormals, many times slower
GROUPS = {
    "far": ("built", "far_1e3", "far_3e4", "far_1e5", "far_1e7"),
    "scaled": ("scale_1e6", "scale_1e10", "scale_1e13", "scale_1e15", "scale_1e-20", "scale_1e-36"),
    "flat": ("flat_centre", "flat_zero", "flat_oblique", "line", "point"),
    "moved": ("mirror_x", "permuted", "neg_zero", "some_collapsed", "built"),
}
assert set(sum(GROUPS.values(), ())) == set(ep.NAMES) - set(ep.REFUSED)


# Rays on which bdpt_trace_rays differs from the host tree walk: none, but for one ray of the "inside" family (drawn inside
# the oblique plane, the scan's triangle ill-conditioned for it: include/bdpt.h "Animated scenes").  The two walks visit
# the same records but shrink their interval in another order, which only shows on such a ray.
DEVICE_OFF = {("courtyard_clipped", "plain", "flat_oblique", "closest"): 1, ("courtyard_clipped", "pieces", "flat_oblique", "closest"): 1}


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _same_float(a, b):
    """bit for bit, any NaN equal to any NaN"""
    return _bits(a) == _bits(b) or (a != a and b != b)


def _context(pkg, which, kind, monkeypatch):
    scene, budgets = ep.fixture(pkg, which)
    if which == "atrium_split":  # the host budgets, for every bdpt_set_scene of the test
        monkeypatch.setenv("BDPT_SPLIT_BUDGET", "1")
        monkeypatch.setenv("BDPT_SPLIT_BUDGET_ALPHA", "4")
    ctx = pkg.Context(0)
    ctx.set_scene(scene.desc)
    host = ep.tree(pkg, which, scene, budgets, kind)
    assert ctx.recs_hash() == host.hash()  # (the same tree to start from)
    if kind == "pieces":
        ctx.prepare(refit_pieces=True)
    return scene, ctx, host


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("kind", ep.KINDS)
@pytest.mark.parametrize("which", ep.SCENES)
def test_device_refit_and_trace_equal_the_host_on_edge_poses(pkg, which, kind, group, monkeypatch):
    scene, ctx, host = _context(pkg, which, kind, monkeypatch)
    updates = 0
    for name in GROUPS[group]:
        c = ep.case(pkg, which, name, N_RAYS_TINY if name in ("scale_1e-20", "scale_1e-36") else N_RAYS)
        host.refit(c.pose.pos)
        ctx.update_geometry(_torch_positions(c.pose.pos))  # device pointer: nothing is inspected on the way
        updates += 1
        assert ctx.recs_hash() == host.hash(), name
        ri, hi = ctx.refit_info(), host.refit_info()
        assert ri.numUpdates == updates and _same_float(ri.sahCost, hi.sahCost) and _same_float(ri.sahCostBuilt, hi.sahCostBuilt), name
        hits = 0
        for m, mode in enumerate(MODES):
            prim, tuv = _trace_device(ctx, c.rays, mode)
            hp, ht = host.trace(c.rays, m, 0)
            # bit for bit the host walk's answer.  Where the SCAN's triangle is ill-conditioned for the ray (the documented
            # limit: its reported point can lie outside its box) the answer depends on the order in which a walk shrinks
            # its interval, and the device's order is not the host's: only such rays may differ, from either.
            off = ((prim >= 0) != (hp >= 0)) if m == 2 else ((prim != hp) | (tuv.view(np.uint32) != ht.view(np.uint32)).any(axis=1))
            assert not (off & ~c.excused(m, off)).any(), (name, mode, "host walk", c.tally(off))
            bad = c.differs(m, prim, tuv)
            assert not (bad & ~c.excused(m, bad)).any(), (name, mode, "scan", c.tally(bad))
            assert int(off.sum()) == DEVICE_OFF.get((which, kind, name, mode), 0), (name, mode, c.tally(off))
            hits += int((prim >= 0).sum())
        assert (hits == 0) == (c.pose.cls == "blind"), (name, hits)
    host.close()
    ctx.close()
    scene.close()


@pytest.mark.parametrize("which", ep.SCENES)
def test_host_memory_update_equals_device_memory_update_far_away(pkg, which, monkeypatch):
    """The host path (checked, copied) on the far pose gives the device path's records."""
    scene, ctx, host = _context(pkg, which, "pieces", monkeypatch)
    c = ep.case(pkg, which, "far_1e5", N_RAYS)
    host.refit(c.pose.pos)
    ctx.update_geometry(c.pose.pos)
    assert ctx.recs_hash() == host.hash()
    host.close()
    ctx.close()
    scene.close()


def test_positions_beyond_the_stated_range_are_refused(pkg, monkeypatch):
    """include/bdpt.h "Animated scenes": |coordinate| <= 2^60.  The pose scaled by 1e19 (finite; the squared diagonal
    overflows) is refused by bdpt_set_scene and by a host-memory update, and the context goes on as it was."""
    scene, ctx, host = _context(pkg, "atrium_split", "plain", monkeypatch)
    c = ep.case(pkg, "atrium_split", "scale_1e19", N_RAYS)
    assert c.pose.cls == "refused" and np.isfinite(c.pose.pos).all()
    before = ctx.recs_hash()
    with pytest.raises(pkg.BdptError, match="beyond 2\\^60"):
        ctx.update_geometry(c.pose.pos)
    assert ctx.recs_hash() == before and ctx.refit_info().numUpdates == 0
    other = pkg.Context(0)
    with pytest.raises(pkg.BdptError, match="beyond 2\\^60"):
        other.set_scene(c.desc)
    other.close()
    edge = np.ascontiguousarray(c.p0 * np.float32(0.999 * 2.0 ** 60 / np.abs(c.p0).max()), np.float32)  # the largest |coordinate| just below 2^60
    assert float(np.abs(edge).max()) <= 2.0 ** 60
    ctx.update_geometry(edge)
    host.refit(edge)
    assert ctx.recs_hash() == host.hash() and np.isfinite(ctx.refit_info().sahCost)
    host.close()
    ctx.close()
    scene.close()


@pytest.mark.parametrize("kind", ep.KINDS)
def test_skinned_updates_with_edge_rigs(pkg, kind, monkeypatch):
    """edge_poses.skin_rigs through bdpt_update_skinned (device bones): the deform pass's output equals the restatement
    on both gather paths (bit for bit; by class where the blend cancels or overflows), and the refitted records and SAH
    cost equal the host refit of bdpt_host_skin's positions.  The overflowing rig comes last: its positions are not
    finite, so its boxes are NaN — no address in the records derives from a position (bvh.h bvhRefitNodeT reads indices,
    childBase and the child offsets only; tests/sanitize/refit_edge_main.cpp runs that arithmetic on the host) — and the
    device must answer every query as the host walk does: with a miss."""
    import skin_numpy as sn
    scene, ctx, host = _context(pkg, "atrium_split", kind, monkeypatch)
    p0 = ep.positions_of(scene.desc)
    c = ep.case(pkg, "atrium_split", "built", N_RAYS)
    lib = pkg.load_library()
    rigs = sorted(ep.skin_rigs(p0), key=lambda r: r.name == "overflowing")  # (stable: the rest keep their order)
    assert rigs[-1].name == "overflowing" and all(np.isfinite(sn.skin(p0, r.W, r.I, r.bones)[0]).all() for r in rigs[:-1])
    for rig in rigs:
        ctx.set_skin(p0, rig.W, rig.I, rig.num_bones)
        ctx.update_skinned(rig.bones)  # host bones: checked, and staged for bdpt_test_skin_kernel below
        ctx.update_skinned(_torch_positions(rig.bones))
        with np.errstate(all="ignore"):
            want, _, _ = sn.skin(p0, rig.W, rig.I, rig.bones)

        def streams(label):
            gp, _, _ = ctx.read_skinned()
            if rig.kind == "bits":
                assert np.array_equal(sn.bits(gp), sn.bits(want)), (rig.name, label, int((sn.bits(gp) != sn.bits(want)).any(axis=1).sum()))
            else:
                assert np.array_equal(ep.value_class(gp), ep.value_class(want)), (rig.name, label)

        streams("update")
        rc, hp, _, _ = sn.host_skin(lib, pkg.abi, p0, rig.W, rig.I, rig.bones)
        assert rc == 0
        host.refit(hp)
        if np.isfinite(hp).all():
            assert ctx.recs_hash() == host.hash(), rig.name
            assert _same_float(ctx.refit_info().sahCost, host.refit_info().sahCost), rig.name
        else:
            assert rig.name == "overflowing"
            for m, mode in enumerate(MODES):
                prim, tuv = _trace_device(ctx, c.rays, mode)
                hp_, ht = host.trace(c.rays, m, 0)
                assert np.array_equal(prim >= 0, hp_ >= 0) and not (prim >= 0).any(), (rig.name, mode)
        for path in (pkg.abi.SKIN_PATH_GLOBAL, pkg.abi.SKIN_PATH_LDS):
            ctx.test_skin_kernel(path)
            streams(f"forced path {path}")
    host.close()
    ctx.close()
    scene.close()


@pytest.mark.parametrize("kind", ep.KINDS)
def test_morphed_updates_with_edge_rigs(pkg, kind, monkeypatch):
    """edge_poses.morph_rigs through bdpt_update_morphed: host weights, then device weights, then the kernel alone on both
    gather paths — the deform pass's output equals the restatement (bit for bit; by class where the base cancels), and the
    refitted records and SAH cost equal the host refit of bdpt_host_morph's positions.  The last rig morphs ahead of a
    collapsing skin."""
    import morph_numpy as mn
    import skin_numpy as sn
    scene, ctx, host = _context(pkg, "atrium_split", kind, monkeypatch)
    p0 = ep.positions_of(scene.desc)
    lib = pkg.load_library()
    for rig in ep.morph_rigs(p0):
        sk = rig.skin
        bones = None if sk is None else sk["bones"]
        if sk is None:
            mn.set_morph(ctx, rig.tg, rig.base)
        else:
            ctx.set_skin(rig.base, sk["W"], sk["I"], len(bones))
            mn.set_morph(ctx, rig.tg)
        want, _, _ = mn.morph(rig.tg, rig.weights, rig.base, rig=sk, bones=bones)

        def streams(label):
            gp = ctx.read_morphed()[0] if sk is None else ctx.read_skinned()[0]
            if rig.kind == "bits":
                assert np.array_equal(sn.bits(gp), sn.bits(want)), (rig.name, label, int((sn.bits(gp) != sn.bits(want)).any(axis=1).sum()))
            else:
                assert np.array_equal(ep.value_class(gp), ep.value_class(want)), (rig.name, label)

        rc, hp, _, _ = mn.host_morph(lib, pkg.abi, rig.tg, rig.weights, rig.base, rig=sk, bones=bones)
        assert rc == 0
        host.refit(hp)
        for label, dev in (("host weights", False), ("device weights", True)):
            w = _torch_positions(rig.weights) if dev else rig.weights
            b = None if bones is None else (_torch_positions(bones) if dev else bones)
            ctx.update_morphed(w, b)
            streams(label)
            assert ctx.recs_hash() == host.hash(), (rig.name, label)
            assert _same_float(ctx.refit_info().sahCost, host.refit_info().sahCost), (rig.name, label)
        for path in (pkg.abi.MORPH_PATH_GLOBAL, pkg.abi.MORPH_PATH_LDS):
            ctx.test_morph_kernel(path)
            streams(f"forced path {path}")
    host.close()
    ctx.close()
    scene.close()


WALK_POSES = ("flat_centre", "far_1e3", "some_collapsed")


@pytest.mark.parametrize("name", WALK_POSES)
@pytest.mark.parametrize("kind", ep.KINDS)
def test_two_step_walk_equals_the_composed_loop_on_edge_poses(pkg, kind, name, monkeypatch):
    """bdpt_walk_query, two steps from the pose's ray batch, on the context refitted to the pose: vertices, info, samples and
    hits equal the loop composed of the single queries, and step 0 is the trace the host walk answers."""
    from test_gpu_walk_query import F, _assert_equal, _run
    from walk_loop import ContextQueries, kinds, walk_loop
    scene, ctx, host = _context(pkg, "atrium_split", kind, monkeypatch)
    c = ep.case(pkg, "atrium_split", name, N_RAYS)
    host.refit(c.pose.pos)
    ctx.update_geometry(_torch_positions(c.pose.pos))
    assert ctx.recs_hash() == host.hash()
    r = c.rays
    n = len(r)
    rng = np.random.default_rng(11)
    starts = np.zeros((n, 12), F)
    starts[:, 0:3], starts[:, 3], starts[:, 4:7], starts[:, 7] = r[:, 0:3], r[:, 6], r[:, 3:6], r[:, 7]
    starts[:, 8:11] = rng.uniform(0.1, 1.0, (n, 3)).astype(F)
    seeds = rng.integers(-2**31, 2**31, n).astype(np.int32)
    min_t = float(r[0, 6])
    for mat in (0, 1):
        want = walk_loop(ContextQueries(ctx, mat, min_t), starts, seeds, 2)
        got = _run(lambda *a, **kw: ctx.walk(*a, mat_index=mat, min_t=min_t, **kw), starts, seeds, 2)
        _assert_equal(got, want, f"{name} {kind} mat {mat}")
        hit0 = got[3][0]
        hp, ht = host.trace(r, 0, 0)
        prim0 = hit0.view(np.int32)[:, 3]
        assert np.array_equal(prim0, hp) and np.array_equal(np.ascontiguousarray(hit0[:, 0:3]).view(np.uint32)[hp >= 0], ht.view(np.uint32)[hp >= 0])
        real, ghost, none = kinds(got[1])
        assert real[0].any() and ghost[0].any()
        assert real[1].any() or name == "flat_centre"  # (one plane: a path that leaves it cannot come back)
    host.close()
    ctx.close()
    scene.close()


class _MovedWithCamera:
    """a scene at a pose: its description there and its camera carried along by `shift`"""

    def __init__(self, scene, desc, shift):
        self.scene, self.desc, self.shift = scene, desc, shift

    def camera(self, aspect):
        cam = self.scene.camera(aspect)
        for k in range(3):
            cam.posW[k] = np.float32(np.float32(cam.posW[k]) + np.float32(self.shift[k]))
        return cam


@pytest.mark.parametrize("name", WALK_POSES)
@pytest.mark.parametrize("kind", ep.KINDS)
def test_frame_on_an_edge_pose_equals_the_oracle_and_a_rebuild(pkg, ob, kind, name, monkeypatch):
    """One 64x36 frame after the update to the pose (the camera carried along with the far pose): equal to the oracle's on the
    posed description and to a fresh context's bdpt_set_scene at the pose, bit for bit, as tests/test_gpu_refit.py does."""
    from test_gpu_configs import _assert_frame_equals_oracle
    from test_gpu_refit import _frame
    if True:  # the host budgets, for every bdpt_set_scene of the test
        monkeypatch.setenv("BDPT_SPLIT_BUDGET", "1")
        monkeypatch.setenv("BDPT_SPLIT_BUDGET_ALPHA", "4")
    c = ep.case(pkg, "atrium_split", name, N_RAYS)
    shift = (c.pose.pos.astype(np.float64) - c.p0).mean(axis=0) if name == "far_1e3" else np.zeros(3)
    W, H, D = 64, 36, 4
    pipe = pkg.FramePipeline(c.scene, W, H, max_depth=D, mat_index=0)
    if kind == "pieces":
        pipe.ctx.prepare(refit_pieces=True)
    posed = _MovedWithCamera(c.scene, c.desc, shift)
    pipe.update_geometry(_torch_positions(c.pose.pos))
    pipe.cam = posed.camera(W / H)
    pipe.ctx.set_camera(pipe.cam)
    gp, p = _frame(pipe)
    img = pipe.output.cpu().numpy().copy()
    assert np.isfinite(img).all() and (img[..., :3] > 0).any(), "the frame must see the posed scene"
    _assert_frame_equals_oracle(pkg, ob, posed, pipe, gp, p, f"{name} {kind}")
    fresh = pkg.FramePipeline(posed, W, H, max_depth=D, mat_index=0)
    fresh.gbuffer_frame, fresh.bdpt_frame = pipe.gbuffer_frame - 1, pipe.bdpt_frame - 1
    _frame(fresh)
    fimg = fresh.output.cpu().numpy()
    assert np.array_equal(img.view(np.uint32), fimg.view(np.uint32)), f"{(img != fimg).any(axis=-1).sum()} pixels differ"
    fresh.close()
    pipe.close()
