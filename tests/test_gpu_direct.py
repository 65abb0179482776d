"""GPU tests of direct lighting (csrc/direct.hip): bdpt_direct_query and bdpt_direct_execute against the CPU yardstick
direct_reference.direct_oracle and against the composed device loop they replace.  Both are direct_reference.direct_compose
over a backend.  bdpt_set_lights keeps a scene's light count, so the loop's one-light tables go to a second context that holds
the same geometry with one light: per light k, set_lights([light k]) -> sample_lights(mat_index=1) -> trace_rays("any"), the
intensity from the pinned restatement.  Every comparison is on words viewed as integers, over every item; two NaNs count as
equal."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch  # (before the library is loaded, as test_gpu_gi.py explains)

import direct_reference as dr
import edge_records as er
from area_scenes import bits
from walk_loop import gpu, host

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
W, H = 64, 48
MIN_T = 1e-4
OUTPUTS = ("color", "visible", "traced")
ITEMS, MISSES, DEAD_RUN = 3000, 64, (1024, 256)  # the dead run covers whole 64-item chunks in the middle of the list


class DeviceBackend:
    """direct_compose's backend from the existing device queries: the composed loop.  ctx1 holds the geometry with ONE light."""

    def __init__(self, ctx1, abi, lights, hints=False):
        self.ctx1, self.abi, self.lights, self.hints, self.num_lights = ctx1, abi, lights, hints, len(lights)
        self.hint_occluded = {}

    def light_ray(self, k, rec):
        self.ctx1.set_lights([self.lights[k]])
        smp = host(self.ctx1.sample_lights(gpu(rec), torch.zeros(len(rec), dtype=torch.int32, device="cuda"), mat_index=1, min_t=MIN_T,
                                           use_hints=self.hints))
        self.hint_occluded[k] = ((smp.view(U)[:, 11] >> 16) & 2) != 0
        return smp[:, 0:8].copy(), smp[:, 4:7].copy(), smp[:, 7].copy()

    def intensity(self, k, rec):
        return dr.light_intensity(self.lights[k], rec[:, 0:3])[1]

    def any_hit(self, rays):
        return host(self.ctx1.trace_rays(gpu(rays), "any")) != 0


def direct_query(ctx, rec, hints=False, alive=None, count=None, fill=-7):
    """one bdpt_direct_query with every optional output -> dict of numpy arrays; fill: what the outputs hold before"""
    n = len(rec)
    col = torch.full((n, 4), float(fill), dtype=torch.float32, device="cuda")
    vis = torch.full((n,), int(fill), dtype=torch.int32, device="cuda")
    trc = torch.full((n,), int(fill), dtype=torch.int32, device="cuda")
    res = ctx.direct_lighting(gpu(rec), alive=None if alive is None else gpu(alive), min_t=MIN_T, use_hints=hints, visible=vis, traced=trc,
                              out=col, count=count)
    assert res[0] is col and res[1] is vis and res[2] is trc
    torch.cuda.synchronize()
    return dict(color=host(col), visible=host(vis).view(U), traced=host(trc).view(U))


def _assert_same(got, want, what, keep=None):
    for name in OUTPUTS:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        if keep is not None:
            g, w = g[keep], w[keep]
        diff = ~dr.same_bits(g, w)
        rows = diff.reshape(len(g), int(np.prod(g.shape[1:]))).any(axis=1)
        assert not rows.any(), f"{what}: {name} differ in {int(rows.sum())} of {len(g)} items, first {int(np.argmax(rows))}: " \
                               f"{g[np.argmax(rows)]} vs {w[np.argmax(rows)]}"


_state = {}
SCENES = {"room": dr.DirectScene, "three": dr.three_light_scene, "sixteen": dr.sixteen_light_scene}


def _scene(pkg, ob, name):
    """a scene's contexts (all its lights; the same geometry with one light), items and yardsticks, made once and shared"""
    if name not in _state:
        sc = SCENES[name](pkg)
        sc1 = dr.DirectScene(pkg, dr.one_light(pkg.abi, sc.lights, 0))
        ctx, ctx1 = pkg.Context(0), pkg.Context(0)
        ctx.set_scene(sc.desc)
        ctx1.set_scene(sc1.desc)
        lib = ob.load_oracle(pkg.abi)
        osc = lib.oracle_scene_create(C.byref(sc.desc))
        rec = sc.records(np.random.default_rng(31), ITEMS, misses=MISSES, dead_run=DEAD_RUN)
        s = dict(scene=sc, scene1=sc1, ctx=ctx, ctx1=ctx1, lib=lib, osc=osc, rec=rec, lights=sc.lights)
        s["oracle"] = dr.direct_oracle(ob, pkg.abi, lib, osc, sc.lights, rec, MIN_T)
        _state[name] = s
    return _state[name]


def _loop_of(pkg, s, hints=False):
    key = "loop_hints" if hints else "loop"
    if key not in s:
        q = DeviceBackend(s["ctx1"], pkg.abi, s["lights"], hints)
        s[key] = dr.direct_compose(q, s["rec"], MIN_T)
        s[key]["hint_occluded"] = q.hint_occluded
        s["ctx1"].set_lights([s["lights"][0]])  # the table the one-light context started with
    return s[key]


@pytest.mark.parametrize("name", list(SCENES))
def test_equals_the_oracle_and_the_loop(pkg, ob, name):
    """(1, 2) 1, 3 and 16 lights; 3,064 items with 64 miss records and a run of 256 dead items in the middle: color, visible and
    traced equal direct_compose over the oracle and over the device queries; every light shadows some item and lights some"""
    s = _scene(pkg, ob, name)
    got = direct_query(s["ctx"], s["rec"])
    want = s["oracle"]
    _assert_same(got, want, f"{name}: the oracle")
    _assert_same(got, _loop_of(pkg, s), f"{name}: the loop")
    lv = want["live"]
    dead = ~lv
    assert dead.sum() >= MISSES + DEAD_RUN[1] and (got["visible"][dead] == 0).all() and (got["traced"][dead] == 0).all()
    assert np.array_equal(bits(got["color"][dead, 0:3]), bits(dr.albedo(s["rec"])[dead])) and (got["color"][:, 3] == 1.0).all()
    for k in range(len(s["lights"])):
        bit = U(1 << k)
        assert (got["traced"][lv] & bit).any(), k
        assert ((got["traced"][lv] & bit) != 0)[(got["visible"][lv] & bit) == 0].all(), k  # only a traced light is shadowed
    assert ((got["traced"] & ~got["visible"]) != 0).any() and ((got["traced"] & got["visible"]) != 0).any()
    # relighting from `visible`: the colour recomputed from the mask and the lights' terms, without a ray
    with np.errstate(all="ignore"):
        total = np.zeros((len(lv), 3), F)
        for k in range(len(s["lights"])):
            sk = ((got["visible"] >> U(k)) & 1).astype(F)
            total = total + (sk * want["ldn"][k])[:, None] * want["inten"][k]
        again = total * (dr.albedo(s["rec"]) / dr.SHADER_PI)
    assert dr.same_bits(again[lv], got["color"][lv, 0:3]).all()


@pytest.mark.parametrize("name", list(SCENES))
def test_hints_change_nothing_but_save_traversals(pkg, ob, name):
    """(3) hints on equals hints off on all three outputs; the composed loop's rays, with bdpt_light_query's hint status, show
    how many traversals a hint saves: more than none in the room, and every hinted ray is one bdpt_trace_rays calls occluded"""
    s = _scene(pkg, ob, name)
    off, on = direct_query(s["ctx"], s["rec"]), direct_query(s["ctx"], s["rec"], hints=True)
    _assert_same(on, off, f"{name}: hints on against off")
    _assert_same(on, s["oracle"], f"{name}: hints on against the oracle")
    loop = _loop_of(pkg, s, hints=True)
    _assert_same(on, loop, f"{name}: hints on against the loop with hints")
    saved = 0
    for k in range(len(s["lights"])):
        hinted = loop["need"][k] & loop["hint_occluded"][k]
        saved += int(hinted.sum())
        assert ((loop["visible"][hinted] >> U(k)) & 1 == 0).all(), k  # the traversal agrees with every hint
        if s["lights"][k].type == pkg.abi.LIGHT_DIRECTIONAL:
            assert not loop["hint_occluded"][k].any()
    traversals = sum(int(m.sum()) for m in loop["need"])
    print(f"{name}: {saved} of {traversals} traversals saved by hints")
    if name == "room":
        assert 0 < saved < traversals


def test_alpha_masked_occluders(pkg, ob):
    """(4) a small courtyard with foliage cards: the alpha test runs inside the any-hit traversal and the hint test"""
    scene = pkg.Scene.courtyard(seed=1, target_triangles=4000, foliage_fraction=0.5)
    d = scene.desc
    alpha = [(d.materials[i].flags >> 17) & 3 for i in range(int(d.numMaterials))]
    assert 1 in alpha, "the scene has no alpha-masked material"
    pipe = pkg.FramePipeline(scene, W, H, max_depth=3, min_t=MIN_T)
    rays = pipe.camera_rays()
    hits = torch.empty((W * H, 4), dtype=torch.float32, device="cuda")
    pipe.trace_rays(rays, "closest", out=hits)
    surf = pipe.shade_hits(rays, hits, normal_map=False)
    torch.cuda.synchronize()
    surf = host(surf)
    lib = ob.load_oracle(pkg.abi)
    osc = lib.oracle_scene_create(C.byref(d))
    lights = (pkg.abi.Light * int(d.numLights))(*[d.lights[i] for i in range(int(d.numLights))])
    want = dr.direct_oracle(ob, pkg.abi, lib, osc, lights, surf, MIN_T)
    for hints in (False, True):
        got = direct_query(pipe.ctx, surf, hints=hints)
        _assert_same(got, want, f"courtyard, hints {hints}: the oracle")
    assert ((got["traced"] & ~got["visible"]) != 0).any() and ((got["traced"] & got["visible"]) != 0).any()
    lib.oracle_scene_destroy(osc)
    torch.cuda.synchronize()
    pipe.close()
    scene.close()


def test_edge_records_beside_ordinary_ones(pkg, ob):
    """(5) edge_records.light_cases — a point at the light and within sqrt(1e-5) of it, distances that over- and underflow,
    N.L == 0, the cone's edge, penumbrae, zero and non-unit dirW, intensities 0, negative, 1e30 and inf — every third record
    with a NaN, zero or non-unit normal, beside ordinary records: equal to the oracle composition, with and without hints,
    but for rays with a direction component below 1e-30 (the ray contract's rule for the tree walk)"""
    lib = ob.load_oracle(pkg.abi)
    nan = F("nan")
    normals = [(nan, 0, 1), (0, 0, 0), (-0.0, 0.0, -0.0), (0, 3.5, 0), (nan, nan, nan), (F("inf"), 0, 0)]
    seen_nan = False
    for count in (1, 3, 4):
        desc, keep = er.two_triangle_scene(pkg.abi, count)
        ctx = pkg.Context(0)
        ctx.set_scene(desc)
        osc = lib.oracle_scene_create(C.byref(desc))
        for c in er.light_cases():
            if len(c.lights) != count:
                continue
            lights = er.make_lights(pkg.abi, c.lights)
            ctx.set_lights(list(lights))
            rec = c.surf.copy()
            for j, i in enumerate(range(1, len(rec), 3)):
                if j % 2:
                    rec[i, 4:7] = np.array(normals[(j // 2) % len(normals)], F)
            with np.errstate(all="ignore"):
                want = dr.direct_oracle(ob, pkg.abi, lib, osc, lights, rec, MIN_T)
                tiny = np.zeros(len(rec), bool)
                for r in want["rays"]:
                    tiny |= ((np.abs(r[:, 4:7]) < 1e-30) & (r[:, 4:7] != 0)).any(axis=1)
            assert tiny.mean() < 0.5, c.name
            for hints in (False, True):
                _assert_same(direct_query(ctx, rec, hints=hints), want, f"{c.name}, hints {hints}", ~tiny)
            seen_nan |= bool(np.isnan(want["color"]).any())
        lib.oracle_scene_destroy(osc)
        torch.cuda.synchronize()
        ctx.close()
    assert seen_nan, "no NaN colour: the infinite intensities never met a shadow or a zero"


def test_item_counts_device_counts_and_alive(pkg, ob):
    """(6, 7) 1, 63, 64, 65, 80 and 4,097 items; a device count below, at and above the capacity with the poisoned outputs beyond
    it untouched; alive bytes that drop every third item; host arrays go to the device and back"""
    s = _scene(pkg, ob, "three")
    ctx = s["ctx"]
    n0 = len(s["rec"])
    rec = s["rec"][np.arange(4097) % n0]
    want = dr.direct_oracle(ob, pkg.abi, s["lib"], s["osc"], s["lights"], rec, MIN_T)
    for n in (1, 63, 64, 65, 80, 4097):
        for hints in (False, True):
            _assert_same(direct_query(ctx, rec[:n], hints=hints), {k: want[k][:n] for k in OUTPUTS}, f"{n} items, hints {hints}")
    n = len(rec)
    for m in (0, 65, 1000, n, n + 9):
        cnt = torch.tensor([m], dtype=torch.int32, device="cuda")
        got = direct_query(ctx, rec, count=cnt, fill=-7)
        k = min(m, n)
        _assert_same({x: got[x][:k] for x in OUTPUTS}, {x: want[x][:k] for x in OUTPUTS}, f"device count {m}")
        assert (got["color"][k:] == -7.0).all() and (got["visible"].view(np.int32)[k:] == -7).all() and \
            (got["traced"].view(np.int32)[k:] == -7).all(), m
    alive = (np.arange(n) % 3 != 1).astype(np.uint8)
    got = direct_query(ctx, rec, alive=alive)
    _assert_same(got, dr.direct_oracle(ob, pkg.abi, s["lib"], s["osc"], s["lights"], rec, MIN_T, alive=alive), "alive")
    dead = alive == 0
    assert np.array_equal(bits(got["color"][dead, 0:3]), bits(dr.albedo(rec)[dead])) and (got["visible"][dead] == 0).all()
    h = ctx.direct_lighting(rec[:65], min_t=MIN_T)
    assert isinstance(h, np.ndarray) and dr.same_bits(h, want["color"][:65]).all()
    only = ctx.direct_lighting(gpu(rec[:65]), min_t=MIN_T, traced=True)
    torch.cuda.synchronize()
    assert len(only) == 2 and np.array_equal(host(only[1]).view(U), want["traced"][:65])


def _gbuffer_items(pipe):
    """the query's inputs for the pass: positions, half-decoded normals, diffuse and specular colours, prim from worldPosition.w"""
    pos = host(pipe.channels["WorldPosition"]).reshape(-1, 4)
    nrm = host(pipe.channels["WorldNormal"].float()).reshape(-1, 4)
    dif = host(pipe.channels["MaterialDiffuse"].float()).reshape(-1, 4)
    spec = host(pipe.channels["MaterialSpecRough"].float()).reshape(-1, 4)
    rec = dr.ar.surface_records(pos[:, 0:3], nrm[:, 0:3], np.where(pos[:, 3] != 0, 0, -1).astype(np.int32))
    rec[:, 12:15], rec[:, 16:19] = dif[:, 0:3], spec[:, 0:3]
    return rec


def test_execute_equals_the_query_and_tiles_reproduce_the_frame(pkg, ob):
    """(8) bdpt_direct_execute equals the query fed the G-buffer on a 64 x 48 frame, with and without hints; a rows tile and a
    stripes context write only their pixels, with the whole frame's values; FramePipeline.direct_lighting is that call"""
    scene = pkg.Scene.cornell()
    pipe = pkg.FramePipeline(scene, W, H, max_depth=3, min_t=MIN_T)
    st = pipe._stream_ptr()
    pipe.ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, st)
    torch.cuda.synchronize()
    img = host(pipe.direct_lighting()).copy()
    assert pipe.last_direct_params.flags == 0 and pipe.channels[pkg.DIRECT_CHANNEL] is not None
    hinted = host(pipe.direct_lighting(use_hints=True)).copy()
    assert pipe.last_direct_params.flags == 1 and dr.same_bits(hinted, img).all()
    rec = _gbuffer_items(pipe)
    got = direct_query(pipe.ctx, rec)
    assert dr.same_bits(img.reshape(-1, 4), got["color"]).all()
    background = rec.view(np.int32)[:, 23] < 0
    assert background.any() and (~background).any() and (img[..., 3] == 1.0).all() and (img[..., 0:3] > 0).any()
    assert np.array_equal(bits(img.reshape(-1, 4)[background, 0:3]), bits(dr.albedo(rec)[background]))
    for kind in ("rows", "stripes"):
        ctx = pkg.Context(0)
        ctx.set_scene(scene.desc)
        if kind == "rows":
            ctx.resize(W, H, 16, 32, 3)
        else:
            ctx.resize_stripes(W, H, 4, 3, 1, 3)
        rows = np.zeros(H, bool)
        for y0, y1 in ctx.row_ranges():
            rows[y0:y1] = True
        assert 0 < rows.sum() < H
        out = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
        ctx.direct_execute(pipe.gb, out, min_t=MIN_T, use_hints=kind == "stripes", stream=st)  # (no camera: the pass needs none)
        torch.cuda.synchronize()
        tile = host(out)
        assert dr.same_bits(tile[rows], img[rows]).all(), kind
        assert (tile[~rows] == -7.0).all(), kind
        ctx.close()
    torch.cuda.synchronize()
    pipe.close()
    scene.close()


def test_after_set_lights_and_a_geometry_update(pkg, ob):
    """(9) the lights move (bdpt_set_lights), then a block moves (bdpt_update_geometry): the outputs follow, with and without
    hints (the lights' cube maps are re-traced), and equal the oracle's on the moved scene"""
    sc = dr.three_light_scene(pkg)
    ctx = pkg.Context(0)
    ctx.set_scene(sc.desc)
    lib = ob.load_oracle(pkg.abi)
    rec = sc.records(np.random.default_rng(77), 2048)
    osc = lib.oracle_scene_create(C.byref(sc.desc))
    before = direct_query(ctx, rec)
    _assert_same(before, dr.direct_oracle(ob, pkg.abi, lib, osc, sc.lights, rec, MIN_T), "before")
    moved = dr.gr.three_lights(pkg.abi)
    moved[0].posW[0], moved[0].posW[2] = -0.5, 0.6
    moved[1].intensity[1] = 0.3
    moved[2].dirW[0], moved[2].dirW[1], moved[2].dirW[2] = 0.0, -1.0, 0.0
    ctx.set_lights(list(moved))
    want = dr.direct_oracle(ob, pkg.abi, lib, osc, moved, rec, MIN_T)
    for hints in (False, True):
        after = direct_query(ctx, rec, hints=hints)
        _assert_same(after, want, f"after set_lights, hints {hints}")
    assert not np.array_equal(bits(after["color"]), bits(before["color"]))
    lib.oracle_scene_destroy(osc)
    pos = sc.pos.copy()
    pos[20:44] += np.array([-0.6, 0.0, 0.3], F)  # the six faces of the short block
    ctx.update_geometry(pos)
    sc.pos[:] = pos
    osc = lib.oracle_scene_create(C.byref(sc.desc))
    want = dr.direct_oracle(ob, pkg.abi, lib, osc, moved, rec, MIN_T)
    for hints in (False, True):
        last = direct_query(ctx, rec, hints=hints)
        _assert_same(last, want, f"after update_geometry, hints {hints}")
    assert not np.array_equal(last["visible"], after["visible"])
    lib.oracle_scene_destroy(osc)
    torch.cuda.synchronize()
    ctx.close()


@pytest.mark.parametrize("hints", [False, True])
def test_captured_direct_query(pkg, ob, hints):
    """(10) direct_lighting alone, captured: exactly one kernel node; replays are identical to the eager run, which is the
    oracle's"""
    from test_gpu_ao import _captured_once
    s = _scene(pkg, ob, "sixteen")
    ctx, n = s["ctx"], len(s["rec"])
    surf = gpu(s["rec"])
    outs = dict(color=torch.zeros((n, 4), dtype=torch.float32, device="cuda"), visible=torch.zeros(n, dtype=torch.int32, device="cuda"),
                traced=torch.zeros(n, dtype=torch.int32, device="cuda"))

    def enqueue(st):
        ctx.direct_lighting(surf, min_t=MIN_T, use_hints=hints, out=outs["color"], visible=outs["visible"], traced=outs["traced"], stream=st)

    eager = _captured_once(enqueue, outs, [0])
    _assert_same({k: host(v).view(U) if v.dtype == torch.int32 else host(v) for k, v in eager.items()}, s["oracle"], "eager")


def test_back_to_back_with_the_other_persistent_kernels(pkg, ob):
    """(11) a trace, an AO query, a GI query, a direct query with and one without hints and the trace again on one stream with
    no synchronise between them: each result equals that of the same sequence with a synchronise after every call, every
    output word is written, and the second trace equals the first: a kernel that left the cursor non-zero would starve the next"""
    s = _scene(pkg, ob, "three")
    ctx, n = s["ctx"], 65
    rec = s["rec"][:n]
    assert (rec.view(np.int32)[:, 23] >= 0).all()
    rays = np.zeros((n, 8), F)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = rec[:, 0:3], F(MIN_T), rec[:, 4:7], F(1e38)
    rays_t, surf_t = gpu(rays), gpu(rec)
    seeds_t = gpu(np.arange(n, dtype=np.int32) * 7919 + 1)

    def outputs():
        f = lambda *shape: torch.full(shape, -7.0, dtype=torch.float32, device="cuda")  # noqa: E731
        i = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device="cuda")  # noqa: E731
        return dict(trace1=f(n, 4), ao=f(n), gi=f(n, 4), direct=f(n, 4), visible=i(n), traced=i(n), direct_h=f(n, 4), visible_h=i(n),
                    traced_h=i(n), trace2=f(n, 4))

    def calls(o, st):
        return [lambda: ctx.trace_rays(rays_t, "closest", out=o["trace1"], stream=st),
                lambda: ctx.ambient_occlusion(surf_t, seeds_t, 2, 0.5, min_t=MIN_T, out=o["ao"], stream=st),
                lambda: ctx.direct_lighting(surf_t, min_t=MIN_T, out=o["direct"], visible=o["visible"], traced=o["traced"], stream=st),
                lambda: ctx.diffuse_gi(surf_t, seeds_t, indirect=True, min_t=MIN_T, out=o["gi"], stream=st),
                lambda: ctx.direct_lighting(surf_t, min_t=MIN_T, use_hints=True, out=o["direct_h"], visible=o["visible_h"],
                                            traced=o["traced_h"], stream=st),
                lambda: ctx.trace_rays(rays_t, "closest", out=o["trace2"], stream=st)]

    alone, together = outputs(), outputs()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        st = C.c_void_p(side.cuda_stream)
        for call in calls(alone, st):
            call()
            side.synchronize()
        for call in calls(together, st):
            call()
        side.synchronize()
    for k in alone:
        assert not (host(alone[k]) == -7).any(), k  # written, every word
        assert np.array_equal(host(together[k]).view(U), host(alone[k]).view(U)), k
    assert np.array_equal(host(alone["trace1"]).view(U), host(alone["trace2"]).view(U))
    for a, b in (("direct", "direct_h"), ("visible", "visible_h"), ("traced", "traced_h")):
        assert np.array_equal(host(alone[a]).view(U), host(alone[b]).view(U))
    assert dr.same_bits(host(alone["direct"]), s["oracle"]["color"][:n]).all()


def test_frames_and_counters_are_unchanged_by_direct_lighting(pkg):
    """(12) frame, direct-lighting calls on the pipeline's stream, frame gives the images of two frames without them, bit for
    bit; the counters and stage times the frame left are unchanged"""
    scene = pkg.Scene.cornell()
    imgs, cnts = [], []
    for with_direct in (True, False):
        pipe = pkg.FramePipeline(scene, W, H, max_depth=4, flags=pkg.abi.PARAM_COUNTERS)
        pipe.ctx.enable_stage_timing(True)
        pipe.render_frame()
        torch.cuda.synchronize()
        first = host(pipe.output).copy()
        if with_direct:
            before, times = pipe.ctx.counters().as_dict(), pipe.ctx.stage_times()
            a1 = host(pipe.direct_lighting()).copy()
            q = direct_query(pipe.ctx, _gbuffer_items(pipe), hints=True)
            a2 = host(pipe.direct_lighting(use_hints=True))
            torch.cuda.synchronize()
            assert (a1[..., 0:3] > 0).any() and (q["color"][:, 0:3] > 0).any() and dr.same_bits(a1, a2).all()
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
    """(13) every error case returns its code in the stated order, bdpt_last_error names the call, and nothing is enqueued: the
    outputs keep their fill"""
    a = pkg.abi
    lib = pkg.load_library()
    scene = pkg.Scene.cornell()
    ctx = pkg.Context(0)
    n = 256
    surf = torch.zeros((n, 24), dtype=torch.float32, device="cuda")
    bytes_ = torch.ones(n, dtype=torch.uint8, device="cuda")
    cnt = torch.full((4,), n, dtype=torch.int32, device="cuda")
    outs = {k: torch.full((n, 4), -7, dtype=torch.int32, device="cuda") for k in ("col", "vis", "trc")}
    img = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
    gpos = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    gnrm = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
    gdif = torch.full((H, W, 4), 0.25, dtype=torch.float16, device="cuda")
    gspec = torch.full((H, W, 4), 0.5, dtype=torch.float16, device="cuda")
    P = dict(sf=surf.data_ptr(), b=bytes_.data_ptr(), n=cnt.data_ptr(), img=img.data_ptr(), gp=gpos.data_ptr(), gn=gnrm.data_ptr(),
             gd=gdif.data_ptr(), gs=gspec.data_ptr(), **{k: t.data_ptr() for k, t in outs.items()})

    def q(h=ctx._h, num=n, cnt=None, flags=0, reserved=0, sf=P["sf"], al=None, col=P["col"], vis=None, trc=None, desc=True):
        d = a.DirectDesc()
        d.num, d.flags, d.numDevice, d.minT, d.reserved = num, flags, cnt, 1e-4, reserved
        d.surfaces, d.alive, d.color, d.visible, d.traced = sf, al, col, vis, trc
        return lib.bdpt_direct_query(h, C.byref(d) if desc else None, None)

    def x(h=ctx._h, flags=0, reserved=(0, 0), gp=P["gp"], gn=P["gn"], gd=P["gd"], gs=P["gs"], out=P["img"], params=True, gbuffer=True):
        p = a.DirectParams()
        p.minT, p.flags, p.reserved[0], p.reserved[1] = 1e-4, flags, reserved[0], reserved[1]
        gb = a.GBuffer()
        gb.worldPosition, gb.worldNormal, gb.materialDiffuse, gb.materialSpecRough = gp, gn, gd, gs
        return lib.bdpt_direct_execute(h, C.byref(p) if params else None, C.byref(gb) if gbuffer else None, out, None)

    assert q() == -2 and b"direct_query" in lib.bdpt_last_error(ctx._h)      # BDPT_E_STATE: no scene
    assert q(flags=8) == -2                                                   # the state comes first
    assert x() == -2 and b"direct_execute" in lib.bdpt_last_error(ctx._h)
    ctx.set_scene(scene.desc)
    assert x() == -2 and b"no size" in lib.bdpt_last_error(ctx._h)           # a scene but no size
    assert x(flags=2) == -2
    bad = [
        q(h=None), q(desc=False), q(flags=a.PARAM_AREA_LIGHTS), q(flags=a.PARAM_AREA_LIGHTS | 1), q(flags=2), q(flags=2**31), q(reserved=1),
        q(num=0, flags=a.PARAM_AREA_LIGHTS), q(num=0, reserved=3),  # (found before the empty call returns)
        q(sf=None), q(sf=P["sf"] + 4), q(col=None), q(col=P["col"] + 4), q(vis=P["vis"] + 1), q(trc=P["trc"] + 2), q(cnt=P["n"] + 2),
    ]
    assert all(rc == -1 for rc in bad), bad
    assert b"direct_query" in lib.bdpt_last_error(ctx._h)
    assert q(num=0, sf=None, col=None) == 0
    ctx.resize(W, H, 0, H, 3)
    bad = [x(h=None), x(params=False), x(gbuffer=False), x(flags=a.PARAM_AREA_LIGHTS), x(flags=2), x(reserved=(1, 0)), x(reserved=(0, 1)),
           x(gp=None), x(gp=P["gp"] + 8), x(gn=None), x(gn=P["gn"] + 4), x(gd=None), x(gd=P["gd"] + 4), x(gs=None), x(gs=P["gs"] + 4),
           x(out=None), x(out=P["img"] + 8)]
    assert all(rc == -1 for rc in bad), bad
    assert b"direct_execute" in lib.bdpt_last_error(ctx._h)
    torch.cuda.synchronize()
    for t in list(outs.values()) + [img]:
        assert (host(t) == -7).all()
    # and the good calls, hints included, with no camera: a zero worldPosition.w is the background, which shows the diffuse channel
    assert q(al=P["b"], vis=P["vis"], trc=P["trc"], cnt=P["n"], flags=1) == 0 and q() == 0 and x() == 0 and x(flags=1) == 0
    torch.cuda.synchronize()
    # (every record at the origin with N = 0: LdotN is 0 for every light, so no ray, every light "visible", a black colour)
    nl = int(scene.desc.numLights)
    assert (host(outs["vis"]).reshape(-1)[:n] == (1 << nl) - 1).all() and (host(outs["trc"]).reshape(-1)[:n] == 0).all()
    col = host(outs["col"]).view(F).reshape(-1, 4)[:n]
    assert (col[:, 0:3] == 0).all() and (col[:, 3] == 1.0).all()
    got = host(img)
    assert (got[..., 0:3] == 0.25).all() and (got[..., 3] == 1.0).all()
    ctx.close()
    scene.close()


def test_cpp_host_direct_equals_the_python_pipeline(pkg, tmp_path):
    """(14) bdpt_render --direct --raw on the Cornell box equals the Python pipeline's G-buffer -> direct lighting image of
    the same frame, bit for bit, with and without --direct-hints; bad combinations are refused"""
    import __graft_entry__ as ge
    exe = os.path.join(ge.PKG_DIR, "host", "bdpt_render")
    assert os.path.exists(exe), "host/bdpt_render not built (run __graft_entry__.build())"
    raw = tmp_path / "direct.f32"
    scene = pkg.Scene.cornell()
    for extra, kw in (([], {}), (["--direct-hints"], dict(use_hints=True))):
        r = subprocess.run([exe, "--scene", "cornell", "--width", str(W), "--height", str(H), "--frames", "3", "--direct"] + extra +
                           ["--out", str(tmp_path / "direct.pfm"), "--raw", str(raw)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "direct lighting" in r.stdout and "mean" in r.stdout
        cpp = np.fromfile(raw, F).reshape(H, W, 4)
        pipe = pkg.FramePipeline(scene, W, H)
        st = pipe._stream_ptr()
        for k in range(3):  # the G-buffer of the host's third frame: its jitter follows the frame counter
            pipe.ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, st)
            pipe.gbuffer_frame += 1
            img = pipe.direct_lighting(**kw)
        torch.cuda.synchronize()
        assert dr.same_bits(cpp, host(img)).all(), extra
        assert (cpp[..., 0:3] > 0).any() and (cpp[..., 3] == 1.0).all()
        pipe.close()
    for args, text in ((["--direct-hints"], "goes with --direct"), (["--direct", "--gpus", "1"], "one GPU"), (["--direct", "--gi"], "--gi")):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and text in r.stderr, (args, r.stderr)
    scene.close()
