"""GPU tests of diffuse GI (csrc/gi.hip): bdpt_gi_query and bdpt_gi_execute against the composed device loop they replace
(light_query -> trace_rays("any") masked by status -> sample_bsdf -> trace_rays("closest") -> shade_hits -> light_query ->
trace_rays("any"), the final arithmetic in numpy on the host) and against the CPU yardstick gi_reference.gi_oracle.  Both are
gi_reference.gi_compose over a backend.  Every comparison is on float words viewed as integers, over every item; two NaNs
count as equal (0 / 0 has the sign of the machine that divides)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch  # (before the library is loaded: run alone, this module would otherwise load the library first, which
#                brings in the system's copy of the HIP runtime beside the one torch ships, and a graph captured on a torch stream
#                from launches made through the other copy cannot be read; a whole-suite collection imports torch anyway)

import gi_reference as gr
from area_scenes import LCG_INV, bits
from walk_loop import gpu, host

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
W, H = 64, 48
MISSES = 64  # miss records appended to the primary hits
MIN_T = 1e-4
ALL_FLAGS = (0, gr.INDIRECT, gr.UNIFORM, gr.INDIRECT | gr.UNIFORM)
OUTPUTS = ("color", "hits", "status", "seeds_out")


class DeviceBackend:
    """gi_compose's backend from the existing device queries of a Context: the composed loop"""

    def __init__(self, ctx, lib, min_t=MIN_T):
        self.ctx, self.lib, self.min_t = ctx, lib, min_t

    def nee(self, rec, seeds):
        so = torch.zeros(len(rec), dtype=torch.int32, device="cuda")
        out = self.ctx.sample_lights(gpu(rec), gpu(np.ascontiguousarray(seeds, U).view(np.int32)), mat_index=1, min_t=self.min_t, seeds_out=so)
        torch.cuda.synchronize()
        return host(out), host(so).view(U).copy()

    def any_hit(self, rays):
        return host(self.ctx.trace_rays(gpu(rays), "any")) != 0

    def closest_hit(self, rays):
        hits = torch.empty((len(rays), 4), dtype=torch.float32, device="cuda")
        self.ctx.trace_rays(gpu(rays), "closest", out=hits)
        return host(hits)

    def cosine_direction(self, rec, seeds):
        return host(self.ctx.sample_bsdf(gpu(rec), gpu(np.ascontiguousarray(seeds, U).view(np.int32)), mat_index=1))[:, 0:3].copy()

    def shade(self, rays, hits, flags):
        return host(self.ctx.shade_hits(gpu(rays), gpu(hits), normal_map=bool(flags & gr.NORMAL_MAP)))


def gi_loop(ctx, lib, rec, seeds, flags, **kw):
    return gr.gi_compose(DeviceBackend(ctx, lib), rec, seeds, flags, MIN_T, **kw)


def gi_query(ctx, rec, seeds, flags, view_pos=None, shade_flags=0, alive=None, count=None, fill=-7):
    """one bdpt_gi_query with every optional output -> dict of numpy arrays; fill: what the outputs hold before"""
    n = len(rec)
    col = torch.full((n, 4), float(fill), dtype=torch.float32, device="cuda")
    hits = torch.full((n, 4), float(fill), dtype=torch.float32, device="cuda")
    status = torch.full((n,), int(fill), dtype=torch.int32, device="cuda")
    sout = torch.full((n,), int(fill), dtype=torch.int32, device="cuda")
    res = ctx.diffuse_gi(gpu(rec), gpu(np.ascontiguousarray(seeds, U).view(np.int32)), indirect=bool(flags & gr.INDIRECT),
                         cosine=not (flags & gr.UNIFORM), view_pos=view_pos, normal_map=bool(shade_flags & gr.NORMAL_MAP), min_t=MIN_T,
                         alive=None if alive is None else gpu(alive), out=col, hits=hits, status=status, seeds_out=sout, count=count)
    assert res is col
    torch.cuda.synchronize()
    return dict(color=host(col), hits=host(hits), status=host(status).view(U), seeds_out=host(sout).view(U))


def _assert_same(got, want, what, keep=None):
    for name in OUTPUTS:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        if keep is not None:
            g, w = g[keep], w[keep]
        diff = ~gr.same_bits(g, w)
        rows = diff.reshape(len(g), int(np.prod(g.shape[1:]))).any(axis=1)
        assert not rows.any(), f"{what}: {name} differ in {int(rows.sum())} of {len(g)} items, first {int(np.argmax(rows))}: " \
                               f"{g[np.argmax(rows)]} vs {w[np.argmax(rows)]}"


def _primary_items(pipe):
    """bdpt_surface records of the pipeline's primary hits with MISSES miss records appended, and one RNG state per item"""
    rays = pipe.camera_rays()
    hits = torch.empty((W * H, 4), dtype=torch.float32, device="cuda")
    pipe.trace_rays(rays, "closest", out=hits)
    surf = pipe.shade_hits(rays, hits, normal_map=False)
    torch.cuda.synchronize()
    surf = host(surf)
    assert 0 < (surf.view(np.int32)[:, 23] >= 0).sum()
    rng = np.random.default_rng(23)
    miss = rng.uniform(-1, 1, (MISSES, 24)).astype(F)
    miss.view(np.int32)[:, 23] = -1 - np.arange(MISSES, dtype=np.int32) % 3
    surf = np.concatenate([surf, miss])
    seeds = rng.integers(0, 2**32, len(surf), dtype=np.uint64).astype(U)
    return surf, seeds


_state = {}


def _cornell(pkg, ob):
    if "cornell" not in _state:
        scene = pkg.Scene.cornell()
        pipe = pkg.FramePipeline(scene, W, H, max_depth=3, min_t=MIN_T)
        surf, seeds = _primary_items(pipe)
        lib = ob.load_oracle(pkg.abi)
        osc = lib.oracle_scene_create(C.byref(scene.desc))
        lights = (pkg.abi.Light * int(scene.desc.numLights))(*[scene.desc.lights[i] for i in range(int(scene.desc.numLights))])
        view = [float(pipe.cam.posW[k]) for k in range(3)]
        _state["cornell"] = dict(scene=scene, pipe=pipe, ctx=pipe.ctx, surf=surf, seeds=seeds, lib=lib, osc=osc, lights=lights, view=view, loops={})
    return _state["cornell"]


def _room(pkg, ob, open_top):
    key = "open" if open_top else "room"
    if key not in _state:
        sc = gr.RoomScene(pkg, open_top=open_top)
        ctx = pkg.Context(0)
        ctx.set_scene(sc.desc)
        lib = ob.load_oracle(pkg.abi)
        osc = lib.oracle_scene_create(C.byref(sc.desc))
        surf, seeds = sc.records(np.random.default_rng(31), 2048, misses=MISSES)
        _state[key] = dict(scene=sc, ctx=ctx, surf=surf, seeds=seeds, lib=lib, osc=osc, lights=sc.lights, view=[0.0, 0.0, 3.0], loops={})
    return _state[key]


def _loop_of(s, flags, view=False, nmap=False):
    """the composed loop's answer on the scene's items, computed once per setting and shared"""
    key = (flags, view, nmap)
    if key not in s["loops"]:
        s["loops"][key] = gi_loop(s["ctx"], s["lib"], s["surf"], s["seeds"], flags | (gr.FROM_VIEW if view else 0),
                                  view_pos=s["view"] if view else None, shade_flags=gr.NORMAL_MAP if nmap else 0)
    return s["loops"][key]


def _oracle_of(pkg, ob, s, flags, view=False, nmap=False, env=None):
    return gr.gi_oracle(ob, pkg.abi, s["lib"], s["osc"], s["lights"], s["surf"], s["seeds"], flags | (gr.FROM_VIEW if view else 0), MIN_T,
                        view_pos=s["view"] if view else None, shade_flags=gr.NORMAL_MAP if nmap else 0, env=env)


@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_equals_the_loop_and_the_oracle(pkg, ob, flags):
    """(1) Cornell primary hits and 64 miss records: all four flag settings x FROM_VIEW x normal map; every output equals the
    composed device loop's and gi_oracle's"""
    s = _cornell(pkg, ob)
    lv = s["surf"].view(np.int32)[:, 23] >= 0
    assert (~lv).sum() >= MISSES
    for view in (False, True):
        for nmap in (False, True):
            got = gi_query(s["ctx"], s["surf"], s["seeds"], flags | (gr.FROM_VIEW if view else 0), view_pos=s["view"] if view else None,
                           shade_flags=gr.NORMAL_MAP if nmap else 0)
            _assert_same(got, _loop_of(s, flags, view, nmap), f"flags {flags} view {view} nmap {nmap}: the loop")
            _assert_same(got, _oracle_of(pkg, ob, s, flags, view, nmap), f"flags {flags} view {view} nmap {nmap}: the oracle")
            draws = 3 if flags & gr.INDIRECT else 1
            assert np.array_equal(got["seeds_out"][lv], gr.ar.lcg_chain(s["seeds"][lv], draws)[:, -1])
            assert np.array_equal(got["seeds_out"][~lv], s["seeds"][~lv]) and (got["status"][~lv] == 0).all()
            assert np.array_equal(bits(got["color"][~lv, 0:3]), bits(s["surf"][~lv, 12:15])) and (got["color"][:, 3] == 1.0).all()
            assert (got["hits"].view(np.int32)[~lv, 3] == -1).all()
            st = got["status"][lv]
            assert (st & gr.DIRECT_OCCLUDED).any() and not (st & gr.DIRECT_OCCLUDED).all()
            if flags & gr.INDIRECT:
                assert (st & gr.BOUNCE_HIT).any() and (st & gr.BOUNCE_OCCLUDED).any()
                assert ((got["hits"].view(np.int32)[lv, 3] >= 0) == ((st & gr.BOUNCE_HIT) != 0)).all()
            else:
                assert (st & ~U(gr.DIRECT_OCCLUDED) == 0).all() and (got["hits"].view(np.int32)[:, 3] == -1).all()


@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_three_lights_and_environments(pkg, ob, flags):
    """(1) the room with blocks under a point, a spot and a directional light: every light is chosen; the room open at the top
    with no environment, a constant one and an 8 x 4 map: at least a tenth of the bounce rays miss"""
    s = _room(pkg, ob, False)
    got = gi_query(s["ctx"], s["surf"], s["seeds"], flags)
    want = _loop_of(s, flags)
    _assert_same(got, want, f"room, flags {flags}: the loop")
    _assert_same(got, _oracle_of(pkg, ob, s, flags), f"room, flags {flags}: the oracle")
    lv = want["live"]
    assert set(np.unique(want["light1"][lv])) == {0, 1, 2}
    if flags & gr.INDIRECT:
        assert set(np.unique(want["light2"][want["traced2"]])) == {0, 1, 2}
    o = _room(pkg, ob, True)
    env_map = gr.env_map_8x4()
    dev_map = gpu(env_map)
    for kind, env in (("none", None), ("constant", np.array([0.5, 0.5, 0.8, 1.0], F)), ("map", env_map)):
        if kind == "none":
            o["ctx"].set_environment()
        elif kind == "constant":
            o["ctx"].set_environment(color=[float(x) for x in env])
        else:
            o["ctx"].set_environment(C.c_void_p(dev_map.data_ptr()), 8, 4)
        got = gi_query(o["ctx"], o["surf"], o["seeds"], flags)
        want = gi_loop(o["ctx"], o["lib"], o["surf"], o["seeds"], flags, env=env)
        keep = ~want["env_ambiguous"]
        assert keep.mean() > 0.98
        _assert_same(got, want, f"open room, {kind}, flags {flags}: the loop", keep)
        _assert_same(got, _oracle_of(pkg, ob, o, flags, env=env), f"open room, {kind}, flags {flags}: the oracle", keep)
        if flags & gr.INDIRECT:
            lv = want["live"]
            missed = (got["status"][lv] & gr.BOUNCE_HIT) == 0
            assert missed.mean() >= 0.1
            if kind == "map":
                assert len(np.unique(bits(got["color"][lv][missed]), axis=0)) > 8
    o["ctx"].set_environment()
    torch.cuda.synchronize()


def test_item_counts_device_counts_and_alive(pkg, ob):
    """(2) 1, 63, 64, 65 and 4097 items; a device count below the capacity with the outputs beyond it untouched; alive bytes
    that drop every third item: (diffuse, 1) and the seed untouched"""
    s = _cornell(pkg, ob)
    ctx, flags = s["ctx"], gr.INDIRECT
    n0 = len(s["surf"])
    pick = np.arange(4097) % n0
    surf, seeds = s["surf"][pick], (s["seeds"][pick] + (np.arange(4097) // n0).astype(U)).astype(U)
    want = gi_loop(ctx, s["lib"], surf, seeds, flags)
    for n in (1, 63, 64, 65, 4097):
        _assert_same(gi_query(ctx, surf[:n], seeds[:n], flags), {k: want[k][:n] for k in OUTPUTS}, f"{n} items")
    n = len(surf)
    for m in (0, 65, 1000, n + 9):
        cnt = torch.tensor([m], dtype=torch.int32, device="cuda")
        got = gi_query(ctx, surf, seeds, flags, count=cnt, fill=-7)
        k = min(m, n)
        _assert_same({x: got[x][:k] for x in OUTPUTS}, {x: want[x][:k] for x in OUTPUTS}, f"device count {m}")
        assert (got["color"][k:] == -7.0).all() and (got["hits"][k:] == -7.0).all(), m
        assert (got["status"].view(np.int32)[k:] == -7).all() and (got["seeds_out"].view(np.int32)[k:] == -7).all(), m
    alive = (np.arange(n) % 3 != 1).astype(np.uint8)
    got = gi_query(ctx, surf, seeds, flags, alive=alive)
    _assert_same(got, gi_loop(ctx, s["lib"], surf, seeds, flags, alive=alive), "alive")
    dead = alive == 0
    assert np.array_equal(bits(got["color"][dead, 0:3]), bits(surf[dead, 12:15])) and (got["color"][dead, 3] == 1.0).all()
    assert np.array_equal(got["seeds_out"][dead], seeds[dead]) and (got["status"][dead] == 0).all()
    # in place: seeds_out may be seeds
    st = gpu(seeds.view(np.int32))
    ctx.diffuse_gi(gpu(surf), st, min_t=MIN_T, seeds_out=st)
    torch.cuda.synchronize()
    assert np.array_equal(host(st).view(U), want["seeds_out"])
    # host arrays go to the device and back
    h = ctx.diffuse_gi(surf[:65], seeds[:65], min_t=MIN_T)
    assert isinstance(h, np.ndarray) and gr.same_bits(h, want["color"][:65]).all()


def test_alpha_masked_occluders_and_bounce_hits(pkg, ob):
    """(3) a small courtyard with foliage cards: the alpha test runs inside the any-hit and the closest-hit traversals"""
    scene = pkg.Scene.courtyard(seed=1, target_triangles=4000, foliage_fraction=0.5)
    d = scene.desc
    alpha = [(d.materials[i].flags >> 17) & 3 for i in range(int(d.numMaterials))]
    assert 1 in alpha, "the scene has no alpha-masked material"
    pipe = pkg.FramePipeline(scene, W, H, max_depth=3, min_t=MIN_T)
    surf, seeds = _primary_items(pipe)
    lib = ob.load_oracle(pkg.abi)
    osc = lib.oracle_scene_create(C.byref(d))
    lights = (pkg.abi.Light * int(d.numLights))(*[d.lights[i] for i in range(int(d.numLights))])
    view = [float(pipe.cam.posW[k]) for k in range(3)]
    for flags in (gr.INDIRECT, gr.INDIRECT | gr.UNIFORM):
        got = gi_query(pipe.ctx, surf, seeds, flags | gr.FROM_VIEW, view_pos=view, shade_flags=gr.NORMAL_MAP)
        _assert_same(got, gi_loop(pipe.ctx, lib, surf, seeds, flags | gr.FROM_VIEW, view_pos=view, shade_flags=gr.NORMAL_MAP), f"courtyard {flags}: the loop")
        _assert_same(got, gr.gi_oracle(ob, pkg.abi, lib, osc, lights, surf, seeds, flags | gr.FROM_VIEW, MIN_T, view_pos=view,
                                       shade_flags=gr.NORMAL_MAP), f"courtyard {flags}: the oracle")
        assert (got["status"] & gr.BOUNCE_HIT).any() and (got["status"] & gr.DIRECT_OCCLUDED).any()
    lib.oracle_scene_destroy(osc)
    torch.cuda.synchronize()
    pipe.close()
    scene.close()


def test_edge_records_beside_ordinary_ones(pkg, ob):
    """(4) N = 0, NaN N, NaN posW, N not unit, non-finite diffuse and a point within sqrt(1e-5) of the light, every fourth item
    of an ordinary batch: equal to the composed loop, and to the oracle but for records whose direction has a component below
    1e-30 (the ray contract's rule for the tree walk); the items beside them are what they are without the edge records"""
    s = _cornell(pkg, ob)
    surf, seeds = s["surf"].copy(), s["seeds"]
    nan, inf = F("nan"), F("inf")
    lp = np.array([s["lights"][0].posW[k] for k in range(3)], F)
    edges = [
        dict(N=(0, 0, 0)), dict(N=(-0.0, 0.0, -0.0)), dict(N=(0, 3.5, 0)), dict(N=(0.1, 0.2, 0.05)), dict(N=(1e-30, 1e-30, 1e-30)),
        dict(N=(nan, 0, 1)), dict(N=(0, nan, 0)), dict(N=(inf, 0, 0)), dict(P=(nan, 100, 100)), dict(P=(100, 100, nan)),
        dict(P=(inf, 100, 100)), dict(D=(nan, 0.5, 0.5)), dict(D=(inf, 0.5, 0.5)), dict(D=(-inf, 0, 1)), dict(D=(0, 0, 0)),
        dict(P=tuple(lp + np.array([0.002, -0.001, 0.001], F))), dict(P=tuple(lp)), dict(N=(nan, nan, nan), P=(nan, nan, nan)),
    ]
    where = np.nonzero(surf.view(np.int32)[:, 23] >= 0)[0][::4]
    assert len(where) >= 4 * len(edges)
    for j, i in enumerate(where):
        e = edges[j % len(edges)]
        for key, cols in (("N", slice(4, 7)), ("P", slice(0, 3)), ("D", slice(12, 15))):
            if key in e:
                surf[i, cols] = np.array(e[key], F)
    with np.errstate(all="ignore"):
        for flags in (gr.INDIRECT, gr.INDIRECT | gr.UNIFORM):
            got = gi_query(s["ctx"], surf, seeds, flags)
            want = gi_loop(s["ctx"], s["lib"], surf, seeds, flags)
            _assert_same(got, want, f"edge records, flags {flags}: the loop")
            orc = gr.gi_oracle(ob, pkg.abi, s["lib"], s["osc"], s["lights"], surf, seeds, flags, MIN_T)
            tiny = ((np.abs(orc["dirs"]) < 1e-30) & (orc["dirs"] != 0)).any(axis=1) | \
                   ((np.abs(orc["ray1"][:, 4:7]) < 1e-30) & (orc["ray1"][:, 4:7] != 0)).any(axis=1) | \
                   ((np.abs(orc["ray2"][:, 4:7]) < 1e-30) & (orc["ray2"][:, 4:7] != 0)).any(axis=1)
            assert not tiny[np.setdiff1d(np.arange(len(surf)), where)].any()
            _assert_same(got, orc, f"edge records, flags {flags}: the oracle", ~tiny)
            # a zero or NaN normal, or a NaN position: the bounce ray misses, after the item's three draws
            for j, i in enumerate(where):
                e = edges[j % len(edges)]
                if e.get("N") in ((0, 0, 0), (-0.0, 0.0, -0.0)) or any(np.isnan(np.array(e.get("N", (0,)) + e.get("P", (0,)), F))):
                    assert (got["status"][i] & gr.BOUNCE_HIT) == 0 and got["hits"].view(np.int32)[i, 3] == -1, (i, e)
                assert got["seeds_out"][i] == gr.ar.lcg_chain(seeds[i:i + 1], 3)[0, -1]
            keep = np.ones(len(surf), bool)
            keep[where] = False
            _assert_same(got, _loop_of(s, flags), "the items beside the edge records", keep)


def _gbuffer_items(pipe, frame_count):
    """the query's inputs for the pass: positions, half-decoded normals and diffuse colours, prim from worldPosition.w, and
    the pass's seeds"""
    pos = host(pipe.channels["WorldPosition"]).reshape(-1, 4)
    nrm = host(pipe.channels["WorldNormal"].float()).reshape(-1, 4)
    dif = host(pipe.channels["MaterialDiffuse"].float()).reshape(-1, 4)
    n = len(pos)
    rec = gr.ar.surface_records(pos[:, 0:3], nrm[:, 0:3], np.where(pos[:, 3] != 0, 0, -1).astype(np.int32))
    rec[:, 12:15] = dif[:, 0:3]
    st, _ = pipe.ctx.test_rng(np.arange(n, dtype=U), np.full(n, frame_count & 0xFFFFFFFF, U), 1)
    back = (st[:, 0].astype(np.uint64) + np.uint64(2**32 - 1013904223)) & np.uint64(0xFFFFFFFF)
    seeds = ((back * np.uint64(LCG_INV)) & np.uint64(0xFFFFFFFF)).astype(U)  # one LCG step back
    assert np.array_equal(gr.lcg(seeds), st[:, 0])
    return rec, seeds


def test_execute_equals_the_query_and_tiles_reproduce_the_frame(pkg, ob):
    """(5) bdpt_gi_execute equals the query fed the G-buffer, shaded from the camera with the normal map; a rows tile and a
    stripes context write only their pixels, with the whole frame's values; frame counters 0x1337 and 0x1338 differ"""
    s = _cornell(pkg, ob)
    pipe, a = s["pipe"], pkg.abi
    st = pipe._stream_ptr()
    pipe.ctx.set_environment(color=(0.5, 0.5, 0.8, 1.0))
    pipe.ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, st)
    torch.cuda.synchronize()
    assert pipe.gi_frame == 0x1337
    images = {}
    for frame, indirect, cosine in ((0x1337, True, True), (0x1337, True, True), (0x1338, True, True), (5, True, False), (6, False, True)):
        pipe.gi_frame = frame
        img = host(pipe.diffuse_gi(indirect, cosine)).copy()
        assert pipe.gi_frame == frame + 1 and pipe.last_gi_params.frameCount == frame
        if frame in images:
            assert np.array_equal(bits(img), bits(images[frame][0]))
        images[frame] = (img, (gr.INDIRECT if indirect else 0) | (0 if cosine else gr.UNIFORM))
    assert not np.array_equal(bits(images[0x1337][0]), bits(images[0x1338][0]))
    for frame, (img, flags) in images.items():
        rec, seeds = _gbuffer_items(pipe, frame)
        got = gi_query(pipe.ctx, rec, seeds, flags | gr.FROM_VIEW, view_pos=s["view"], shade_flags=gr.NORMAL_MAP)
        assert gr.same_bits(img.reshape(-1, 4), got["color"]).all(), frame
        background = rec.view(np.int32)[:, 23] < 0
        assert background.any() and np.array_equal(bits(img.reshape(-1, 4)[background, 0:3]), bits(rec[background, 12:15]))
        assert (img[..., 3] == 1.0).all()
    p = a.GiParams(0x1337, MIN_T, gr.INDIRECT, 0)
    for kind in ("rows", "stripes"):
        ctx = pkg.Context(0)
        ctx.set_scene(s["scene"].desc)
        if kind == "rows":
            ctx.resize(W, H, 16, 32, 3)
        else:
            ctx.resize_stripes(W, H, 4, 3, 1, 3)
        ctx.set_camera(pipe.cam)
        ctx.set_environment(color=(0.5, 0.5, 0.8, 1.0))
        rows = np.zeros(H, bool)
        for y0, y1 in ctx.row_ranges():
            rows[y0:y1] = True
        assert 0 < rows.sum() < H
        out = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
        ctx.gi_execute(p, pipe.gb, C.c_void_p(out.data_ptr()), st)
        torch.cuda.synchronize()
        got = host(out)
        assert gr.same_bits(got[rows], images[0x1337][0][rows]).all(), kind
        assert (got[~rows] == -7.0).all(), kind
        ctx.close()
    pipe.ctx.set_environment()


def test_after_a_geometry_update(pkg, ob):
    """(6) the short box moves (bdpt_update_geometry): the answer equals that of a fresh context's bdpt_set_scene at the pose,
    and differs from before"""
    scene = pkg.Scene.cornell()
    pipe = pkg.FramePipeline(scene, W, H, max_depth=3, min_t=MIN_T)
    s = _cornell(pkg, ob)
    surf, seeds, flags = s["surf"], s["seeds"], gr.INDIRECT
    before = gi_query(pipe.ctx, surf, seeds, flags)
    _assert_same(before, _loop_of(s, flags), "before the update")
    d = scene.desc
    n = int(d.numVertices)
    pos = np.ctypeslib.as_array(d.positions, (n, 3)).copy()
    moved = pos.copy()
    moved[24:44] += np.array([-40.0, 0.0, -30.0], F)  # the five quads of the short block
    pipe.update_geometry(moved)
    after = gi_query(pipe.ctx, surf, seeds, flags)
    assert not np.array_equal(bits(after["color"]), bits(before["color"])) and np.array_equal(after["seeds_out"], before["seeds_out"])
    np.ctypeslib.as_array(d.positions, (n, 3))[:] = moved
    fresh = pkg.Context(0)
    fresh.set_scene(d)
    _assert_same(after, gi_query(fresh, surf, seeds, flags), "after the update: a fresh context at the pose")
    np.ctypeslib.as_array(d.positions, (n, 3))[:] = pos
    torch.cuda.synchronize()
    fresh.close()
    pipe.close()
    scene.close()


def test_captured_gbuffer_and_gi_execute(pkg, ob):
    """(7) gbuffer_execute -> gi_execute captured into one graph: the G-buffer pass's kernel node and exactly one more for the
    GI call, nothing else; replays are identical to the eager run"""
    from test_gpu_ao import _captured_once
    s = _cornell(pkg, ob)
    pipe = s["pipe"]
    gp, p = pipe.gbuffer_params(), pkg.abi.GiParams(0x1339, MIN_T, gr.INDIRECT, 0)
    img = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")

    def enqueue(st):
        pipe.ctx.gbuffer_execute(gp, pipe.gb, st)
        pipe.ctx.gi_execute(p, pipe.gb, C.c_void_p(img.data_ptr()), st)

    eager = _captured_once(enqueue, dict(img=img), [0, 0])
    got = host(eager["img"])
    assert (got[..., 3] == 1.0).all() and (got[..., 0:3] > 0).any()


def test_captured_gi_query(pkg, ob):
    """(7) gi_query alone, captured: exactly one kernel node; replays are identical to the eager run, which is the loop's"""
    from test_gpu_ao import _captured_once
    s = _cornell(pkg, ob)
    ctx, n = s["ctx"], len(s["surf"])
    surf, seeds = gpu(s["surf"]), gpu(s["seeds"].view(np.int32))
    outs = dict(color=torch.zeros((n, 4), dtype=torch.float32, device="cuda"), hits=torch.zeros((n, 4), dtype=torch.float32, device="cuda"),
                status=torch.zeros(n, dtype=torch.int32, device="cuda"), seeds_out=torch.zeros(n, dtype=torch.int32, device="cuda"))

    def enqueue(st):
        ctx.diffuse_gi(surf, seeds, min_t=MIN_T, normal_map=False, out=outs["color"], hits=outs["hits"], status=outs["status"],
                       seeds_out=outs["seeds_out"], stream=st)

    eager = _captured_once(enqueue, outs, [0])
    _assert_same({k: host(v).view(U) if v.dtype == torch.int32 else host(v) for k, v in eager.items()}, _loop_of(s, gr.INDIRECT), "eager")


def test_frames_and_counters_are_unchanged_by_gi(pkg):
    """(8) frame, GI calls on the pipeline's stream, frame gives the images of two frames without them, bit for bit; the
    counters and stage times the frame left are unchanged"""
    scene = pkg.Scene.cornell()
    imgs, cnts = [], []
    for with_gi in (True, False):
        pipe = pkg.FramePipeline(scene, W, H, max_depth=4, flags=pkg.abi.PARAM_COUNTERS)
        pipe.ctx.enable_stage_timing(True)
        pipe.render_frame()
        torch.cuda.synchronize()
        first = host(pipe.output).copy()
        if with_gi:
            before, times = pipe.ctx.counters().as_dict(), pipe.ctx.stage_times()
            a1 = host(pipe.diffuse_gi()).copy()
            surf, seeds = _primary_items(pipe)
            q = gi_query(pipe.ctx, surf, seeds, gr.INDIRECT | gr.UNIFORM)
            a2 = host(pipe.diffuse_gi(indirect=False))
            torch.cuda.synchronize()
            assert (a1[..., 0:3] > 0).any() and (q["color"][:, 0:3] > 0).any() and (a2[..., 0:3] > 0).any()
            assert pipe.ctx.counters().as_dict() == before
            assert pipe.ctx.stage_times() == times
        pipe.render_frame()
        torch.cuda.synchronize()
        imgs.append((first, host(pipe.output).copy()))
        cnts.append(pipe.ctx.counters().as_dict())
        pipe.close()
    for x, y in zip(imgs[0], imgs[1]):
        assert np.array_equal(bits(x), bits(y))
    assert cnts[0] == cnts[1]
    scene.close()


def test_error_cases_through_the_c_abi(pkg):
    """(9) every error case returns its code in the stated order, bdpt_last_error names the call, and nothing is enqueued: the
    outputs keep their fill"""
    a = pkg.abi
    lib = pkg.load_library()
    scene = pkg.Scene.cornell()
    ctx = pkg.Context(0)
    n = 256
    surf = torch.zeros((n, 24), dtype=torch.float32, device="cuda")
    seeds = torch.zeros(n, dtype=torch.int32, device="cuda")
    bytes_ = torch.ones(n, dtype=torch.uint8, device="cuda")
    cnt = torch.full((4,), n, dtype=torch.int32, device="cuda")
    outs = {k: torch.full((n, 4), -7, dtype=torch.int32, device="cuda") for k in ("col", "hit", "st", "so")}
    img = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
    gpos = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    gnrm = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
    gdif = torch.full((H, W, 4), 0.25, dtype=torch.float16, device="cuda")
    P = dict(sf=surf.data_ptr(), sd=seeds.data_ptr(), b=bytes_.data_ptr(), n=cnt.data_ptr(), img=img.data_ptr(), gp=gpos.data_ptr(),
             gn=gnrm.data_ptr(), gd=gdif.data_ptr(), **{k: t.data_ptr() for k, t in outs.items()})

    def q(h=ctx._h, num=n, cnt=None, flags=1, shade=0, reserved=0, sf=P["sf"], sd=P["sd"], al=None, col=P["col"], hit=None, st=None, so=None,
          desc=True):
        d = a.GiDesc()
        d.num, d.flags, d.numDevice, d.shadeFlags, d.minT, d.reserved = num, flags, cnt, shade, 1e-4, reserved
        d.surfaces, d.seeds, d.alive, d.color, d.hits, d.status, d.seedsOut = sf, sd, al, col, hit, st, so
        return lib.bdpt_gi_query(h, C.byref(d) if desc else None, None)

    def x(h=ctx._h, flags=1, reserved=0, gp=P["gp"], gn=P["gn"], gd=P["gd"], out=P["img"], params=True, gbuffer=True):
        p = a.GiParams(0x1337, 1e-4, flags, reserved)
        gb = a.GBuffer()
        gb.worldPosition, gb.worldNormal, gb.materialDiffuse = gp, gn, gd
        return lib.bdpt_gi_execute(h, C.byref(p) if params else None, C.byref(gb) if gbuffer else None, out, None)

    assert q() == -2 and b"gi_query" in lib.bdpt_last_error(ctx._h)      # BDPT_E_STATE: no scene
    assert q(flags=8) == -2                                               # the state comes first
    assert x() == -2 and b"gi_execute" in lib.bdpt_last_error(ctx._h)
    ctx.set_scene(scene.desc)
    assert x() == -2 and b"no size" in lib.bdpt_last_error(ctx._h)       # a scene but no size
    ctx.resize(W, H, 0, H, 3)
    assert x() == -2 and b"no camera" in lib.bdpt_last_error(ctx._h)     # a size but no camera
    assert x(flags=4) == -2
    bad = [
        q(h=None), q(desc=False), q(flags=8), q(flags=2**31), q(shade=2), q(reserved=1),
        q(num=0, flags=8), q(num=0, shade=4), q(num=0, reserved=3),  # (found before the empty call returns)
        q(sf=None), q(sf=P["sf"] + 4), q(sd=None), q(sd=P["sd"] + 2), q(col=None), q(col=P["col"] + 4), q(hit=P["hit"] + 8),
        q(st=P["st"] + 1), q(so=P["so"] + 2), q(cnt=P["n"] + 2),
    ]
    assert all(rc == -1 for rc in bad), bad
    assert b"gi_query" in lib.bdpt_last_error(ctx._h)
    assert q(num=0, sf=None, sd=None, col=None) == 0
    cam = a.Camera()
    cam.posW[2] = 3.0
    ctx.set_camera(cam)
    bad = [x(h=None), x(params=False), x(gbuffer=False), x(flags=4), x(flags=8), x(reserved=1), x(gp=None), x(gp=P["gp"] + 8), x(gn=None),
           x(gn=P["gn"] + 4), x(gd=None), x(gd=P["gd"] + 4), x(out=None), x(out=P["img"] + 8)]
    assert all(rc == -1 for rc in bad), bad
    assert b"gi_execute" in lib.bdpt_last_error(ctx._h)
    torch.cuda.synchronize()
    for t in list(outs.values()) + [img]:
        assert (host(t) == -7).all()
    # and the good calls: a zero worldPosition.w is the background, which shows the diffuse channel
    assert q(al=P["b"], hit=P["hit"], st=P["st"], so=P["so"], cnt=P["n"]) == 0 and q() == 0 and x() == 0
    torch.cuda.synchronize()
    # (every record at the origin with N = 0 and a zero diffuse: no light term, and the bounce ray misses after three draws)
    assert (host(outs["so"]).reshape(-1)[:n].view(U) == gr.ar.lcg_chain(np.zeros(1, U), 3)[0, -1]).all()
    assert (host(outs["hit"])[:, 3] == -1).all() and (host(outs["st"]).reshape(-1)[:n] == 0).all()
    got = host(img)
    assert (got[..., 0:3] == 0.25).all() and (got[..., 3] == 1.0).all()
    ctx.close()
    scene.close()


def test_cpp_host_gi_equals_the_python_pipeline(pkg, tmp_path):
    """(10) bdpt_render --gi --raw on the Cornell box over 3 frames equals the Python pipeline's G-buffer -> GI -> accumulate
    image, bit for bit; --gi-uniform and --gi-direct-only reach the pass"""
    import __graft_entry__ as ge
    exe = os.path.join(ge.PKG_DIR, "host", "bdpt_render")
    assert os.path.exists(exe), "host/bdpt_render not built (run __graft_entry__.build())"
    raw = tmp_path / "gi.f32"
    scene = pkg.Scene.cornell()
    for extra, kw in (([], {}), (["--gi-uniform"], dict(cosine=False)), (["--gi-direct-only"], dict(indirect=False))):
        r = subprocess.run([exe, "--scene", "cornell", "--width", str(W), "--height", str(H), "--frames", "3", "--gi"] + extra +
                           ["--out", str(tmp_path / "gi.pfm"), "--raw", str(raw)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "mean" in r.stdout
        cpp = np.fromfile(raw, F).reshape(H, W, 4)
        pipe = pkg.FramePipeline(scene, W, H)
        env = torch.tensor(pipe.env_color, dtype=torch.float32, device="cuda").repeat(128, 128, 1).contiguous()
        pipe.ctx.set_environment(C.c_void_p(env.data_ptr()), 128, 128)  # the host's default "EnvironmentMap" channel
        st = pipe._stream_ptr()
        acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        for k in range(3):
            pipe.ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, st)
            pipe.gbuffer_frame += 1
            img = pipe.diffuse_gi(**kw)
            pipe.ctx.accumulate(C.c_void_p(acc.data_ptr()), C.c_void_p(img.data_ptr()), k, pipe.accum_limit, W * H, st)
        torch.cuda.synchronize()
        assert pipe.last_gi_params.frameCount == 0x1339
        assert gr.same_bits(cpp, host(img)).all(), extra
        pipe.close()
    for args, text in ((["--gi-uniform"], "go with --gi"), (["--gi", "--gpus", "1"], "one GPU"), (["--gi", "--ao", "4"], "--gi")):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and text in r.stderr, (args, r.stderr)
    scene.close()
