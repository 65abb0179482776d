"""GPU tests of resampled direct lighting (csrc/ris.hip): bdpt_ris_query and bdpt_ris_execute against the definition,
ris_reference.ris_compose, over the CPU oracle and over the composed device loop the call replaces: per candidate
Context.sample_lights(seeds_out=) and a draw, per sample Context.trace_rays("any") for the survivors.  Every comparison is on
words viewed as integers, over every item; two NaNs count as equal."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch  # (before the library is loaded, as test_gpu_gi.py explains)

import direct_reference as dr
import edge_records as er
import ris_reference as rr
from area_scenes import AreaScene, bits
from walk_loop import gpu, host

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
W, H = 64, 48
MIN_T = 1e-4
FLT_MAX = rr.FLT_MAX
OUTPUTS = ("color", "seeds_out", "traced", "reservoirs")
ITEMS, MISSES, DEAD_RUN = 3000, 64, (1024, 256)  # the dead run covers whole 64-item chunks in the middle of the list
MK = ((1, 1), (2, 1), (8, 3), (32, 2))


class DeviceBackend:
    """ris_compose's backend from the existing device queries: the composed loop"""

    def __init__(self, ctx, mat, area=False, min_t=MIN_T):
        self.ctx, self.mat, self.area, self.min_t = ctx, mat, area, min_t
        self._rec = (None, None)

    def _gpu_rec(self, rec):
        if self._rec[0] is not rec:
            self._rec = (rec, gpu(rec))
        return self._rec[1]

    def _sample(self, rec, states, hints):
        so = torch.empty(len(rec), dtype=torch.int32, device="cuda")
        smp = self.ctx.sample_lights(self._gpu_rec(rec), gpu(states.view(np.int32)), mat_index=self.mat, min_t=self.min_t,
                                     area_lights=self.area, use_hints=hints, seeds_out=so)
        return host(smp), host(so).view(U)

    def candidates(self, rec, states):
        smp, after = self._sample(rec, states, False)
        word = smp.view(U)[:, 11]
        return smp[:, 0:8].copy(), smp[:, 8:11].copy(), word & U(0xFFFF), word >> U(16), after

    def any_hit(self, rays):
        return host(self.ctx.trace_rays(gpu(rays), "any")) != 0

    def hint_occluded(self, rec, states):
        smp, _ = self._sample(rec, states, True)
        return ((smp.view(U)[:, 11] >> U(16)) & U(2)) != 0


def ris_query(ctx, rec, seeds, M, K, mat=1, area=False, hints=False, clamp=FLT_MAX, alive=None, count=None, fill=-7, min_t=MIN_T):
    """one bdpt_ris_query with every optional output -> dict of numpy arrays; fill: what the outputs hold before"""
    n = len(rec)
    col = torch.full((n, 4), float(fill), dtype=torch.float32, device="cuda")
    so, trc = (torch.full((n,), int(fill), dtype=torch.int32, device="cuda") for _ in range(2))
    rsv = torch.full((n, K, 4), int(fill), dtype=torch.int32, device="cuda")
    res = ctx.ris_lighting(gpu(rec), gpu(np.ascontiguousarray(seeds).view(np.int32)), M, K, mat_index=mat, area_lights=area, use_hints=hints,
                           clamp=clamp, min_t=min_t, alive=None if alive is None else gpu(alive), out=col, seeds_out=so, traced=trc,
                           reservoirs=rsv, count=count)
    assert res is col
    torch.cuda.synchronize()
    return dict(color=host(col), seeds_out=host(so).view(U), traced=host(trc).view(U), reservoirs=host(rsv).view(U))


def _assert_same(got, want, what, keep=None, outputs=OUTPUTS):
    for name in outputs:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        if keep is not None:
            g, w = g[keep], w[keep]
        assert g.shape == w.shape, (what, name)
        if not len(g):
            continue
        diff = ~dr.same_bits(g, w) if g.dtype == F else g != w
        rows = diff.reshape(len(g), -1).any(axis=1)
        assert not rows.any(), f"{what}: {name} differ in {int(rows.sum())} of {len(g)} items, first {int(np.argmax(rows))}: " \
                               f"{g[np.argmax(rows)]} vs {w[np.argmax(rows)]}"


_state = {}
SCENES = {"room": dr.DirectScene, "three": dr.three_light_scene, "sixteen": dr.sixteen_light_scene}


def _scene(pkg, ob, name):
    """a scene's context, items, seeds and oracle handle, made once and shared"""
    if name not in _state:
        sc = SCENES[name](pkg)
        ctx = pkg.Context(0)
        ctx.set_scene(sc.desc)
        lib = ob.load_oracle(pkg.abi)
        osc = lib.oracle_scene_create(C.byref(sc.desc))
        rng = np.random.default_rng(31)
        rec = rr.with_view(sc.records(rng, ITEMS, misses=MISSES, dead_run=DEAD_RUN), rng)
        seeds = rng.integers(0, 2**32, len(rec), dtype=np.uint64).astype(U)
        _state[name] = dict(scene=sc, ctx=ctx, lib=lib, osc=osc, rec=rec, seeds=seeds, lights=sc.lights)
    return _state[name]


@pytest.mark.parametrize("mat", [1, 0])
@pytest.mark.parametrize("name", list(SCENES))
def test_equals_the_oracle_and_the_loop(pkg, ob, name, mat):
    """(1) 1, 3 and 16 lights; 3,064 items with 64 miss records and a run of 256 dead items in the middle; (M, K) = (1, 1),
    (2, 1), (8, 3), (32, 2): color, seeds_out, traced and reservoirs equal ris_compose over the oracle and over the device
    queries.  With hints color and seeds_out equal the run without, traced only drops, and where it dropped a reservoir of
    the item carries the hint bit; the composed loop with bdpt_light_query's hint bit gives the same words."""
    s = _scene(pkg, ob, name)
    ctx, rec, seeds = s["ctx"], s["rec"], s["seeds"]
    oracle = rr.OracleBackend(ob, pkg.abi, s["lib"], s["osc"], s["lights"], mat, MIN_T)
    loop = DeviceBackend(ctx, mat)
    saved = 0
    for M, K in MK:
        what = f"{name} mat {mat} M {M} K {K}"
        got = ris_query(ctx, rec, seeds, M, K, mat)
        want = rr.ris_compose(oracle, rec, seeds, M, K, min_t=MIN_T)
        _assert_same(got, want, what + ": the oracle")
        if (M, K) != (32, 2) or name == "sixteen":  # (the loop's 64 + 2 device calls a case: once is enough for M = 32)
            _assert_same(got, rr.ris_compose(loop, rec, seeds, M, K, min_t=MIN_T), what + ": the loop")
        lv = want["live"]
        assert (~lv).sum() >= MISSES + DEAD_RUN[1] and (got["traced"][~lv] == 0).all() and np.array_equal(got["seeds_out"][~lv], seeds[~lv])
        assert np.array_equal(bits(got["color"][~lv, 0:3]), bits(rec[~lv, 12:15])) and (got["color"][:, 3] == 1.0).all()
        status = got["reservoirs"][lv, :, 0] >> U(16)
        assert (status == rr.STATUS_RAY).any() and (status == (rr.STATUS_RAY | rr.STATUS_OCCLUDED)).any(), what  # lit and shadowed
        assert (got["traced"][lv] == (status & 1).sum(axis=1)).all()
        on = ris_query(ctx, rec, seeds, M, K, mat, hints=True)
        _assert_same(on, got, what + ": hints on against off", outputs=("color", "seeds_out"))
        assert (on["traced"] <= got["traced"]).all()
        hinted = ((on["reservoirs"][:, :, 0] >> U(16)) & U(rr.STATUS_HINT_OCCLUDED)) != 0
        assert np.array_equal(got["traced"] - on["traced"], hinted.sum(axis=1).astype(U)), what
        # a hinted sample is one the traversal calls occluded; everything but the two answer bits is unchanged
        off_status = got["reservoirs"][:, :, 0] >> U(16)
        assert ((off_status[hinted] & rr.STATUS_OCCLUDED) != 0).all()
        mask = ~U((rr.STATUS_HINT_OCCLUDED | rr.STATUS_OCCLUDED) << 16)
        assert np.array_equal(on["reservoirs"][:, :, 0] & mask, got["reservoirs"][:, :, 0] & mask)
        assert np.array_equal(on["reservoirs"][:, :, 1:], got["reservoirs"][:, :, 1:])
        if (M, K) == (8, 3):
            _assert_same(on, rr.ris_compose(loop, rec, seeds, M, K, min_t=MIN_T, hints=True), what + ": the loop with hints")
        saved += int(hinted.sum())
    print(f"{name} mat {mat}: {saved} traversals saved by hints")
    if name == "room":
        assert saved > 0


@pytest.mark.parametrize("mat", [1, 0])
def test_area_lights_are_one_more_candidate_source(pkg, ob, mat):
    """(2) the Cornell box with its emissive patch, a textured and an alpha-masked emitter, a point light, a spot light, a
    second point light and a directional light; M = 1 and 8: equal to the composed loop with area_lights=True and, for the
    Lambertian material, to the oracle composition (table candidates from oracle_area_light_sample mode 1; the GGX value of a
    table sample has no restatement outside the device code); some item selects the table and some a light"""
    cornell = pkg.Scene.cornell()
    sc = AreaScene(pkg, cornell, point_light=True, relit=True)
    pipe = pkg.FramePipeline(sc, W, H, max_depth=3, min_t=MIN_T)
    ctx = pipe.ctx
    rays = pipe.camera_rays()
    hits = torch.empty((W * H, 4), dtype=torch.float32, device="cuda")
    pipe.trace_rays(rays, "closest", out=hits)
    rec = host(pipe.shade_hits(rays, hits, normal_map=False))[::2].copy()
    torch.cuda.synchronize()
    seeds = np.random.default_rng(5).integers(0, 2**32, len(rec), dtype=np.uint64).astype(U)
    nl = int(sc.desc.numLights)
    loop = DeviceBackend(ctx, mat, area=True)
    lib = ob.load_oracle(pkg.abi)
    osc = lib.oracle_scene_create(C.byref(sc.desc))
    lights = (pkg.abi.Light * nl)(*[sc.desc.lights[i] for i in range(nl)])
    for M, K, hints in ((1, 1, False), (8, 2, False), (8, 2, True)):
        got = ris_query(ctx, rec, seeds, M, K, mat, area=True, hints=hints)
        if mat == 1 and not hints:
            oracle = rr.OracleBackend(ob, pkg.abi, lib, osc, lights, 1, MIN_T, area=True)
            assert oracle.table
            _assert_same(got, rr.ris_compose(oracle, rec, seeds, M, K, min_t=MIN_T), f"area M {M} K {K}: the oracle")
        _assert_same(got, rr.ris_compose(loop, rec, seeds, M, K, min_t=MIN_T, hints=hints), f"area mat {mat} M {M} K {K} hints {hints}")
        light = got["reservoirs"][:, :, 0] & U(0xFFFF)
        assert (light == nl).any() and (light < nl).any(), "the table and a light are both selected"
        assert (light[light != rr.NO_LIGHT] <= nl).all()
    plain = ris_query(ctx, rec, seeds, 8, 2, mat)
    assert not np.array_equal(bits(plain["color"]), bits(got["color"]))
    lib.oracle_scene_destroy(osc)
    torch.cuda.synchronize()
    pipe.close()
    cornell.close()


def test_item_counts_device_counts_and_alive(pkg, ob):
    """(3) a device count below the capacity leaves the outputs beyond it untouched; 0, 1 and 65 items; an alive mask that
    drops every third item and one that kills every item; seeds_out in place; host arrays"""
    s = _scene(pkg, ob, "three")
    ctx, rec, seeds = s["ctx"], s["rec"], s["seeds"]
    M, K, mat = 4, 2, 1
    want = rr.ris_compose(rr.OracleBackend(ob, pkg.abi, s["lib"], s["osc"], s["lights"], mat, MIN_T), rec, seeds, M, K, min_t=MIN_T)
    n = len(rec)
    for m in (1, 63, 64, 65):
        _assert_same(ris_query(ctx, rec[:m], seeds[:m], M, K, mat), {k: want[k][:m] for k in OUTPUTS}, f"{m} items")
    empty = ctx.ris_lighting(gpu(rec[:0]), gpu(seeds[:0].view(np.int32)), M, K)
    assert tuple(empty.shape) == (0, 4)
    for m in (0, 1, 65, 1000, n, n + 9):
        cnt = torch.tensor([m], dtype=torch.int32, device="cuda")
        got = ris_query(ctx, rec, seeds, M, K, mat, count=cnt)
        k = min(m, n)
        _assert_same({x: got[x][:k] for x in OUTPUTS}, {x: want[x][:k] for x in OUTPUTS}, f"device count {m}")
        assert (got["color"][k:] == -7.0).all() and all((got[x].view(np.int32)[k:] == -7).all() for x in OUTPUTS[1:]), m
    for alive in ((np.arange(n) % 3 != 1).astype(np.uint8), np.zeros(n, np.uint8)):
        got = ris_query(ctx, rec, seeds, M, K, mat, alive=alive)
        _assert_same(got, rr.ris_compose(rr.OracleBackend(ob, pkg.abi, s["lib"], s["osc"], s["lights"], mat, MIN_T), rec, seeds, M, K,
                                         min_t=MIN_T, alive=alive), "alive")
        dead = alive == 0
        assert np.array_equal(bits(got["color"][dead, 0:3]), bits(rec[dead, 12:15])) and np.array_equal(got["seeds_out"][dead], seeds[dead])
        assert (got["reservoirs"][dead, :, 0] == rr.NO_LIGHT).all() and not got["reservoirs"][dead, :, 1:].any()
    st = gpu(seeds.view(np.int32))
    ctx.ris_lighting(gpu(rec), st, M, K, seeds_out=st)
    torch.cuda.synchronize()
    assert np.array_equal(host(st).view(U), want["seeds_out"])
    h = ctx.ris_lighting(rec[:65], seeds[:65], M, K)
    assert isinstance(h, np.ndarray) and dr.same_bits(h, want["color"][:65]).all()


def test_edge_records_beside_ordinary_ones(pkg):
    """(4) edge_records.light_cases — a point at the light and within sqrt(1e-5) of it, distances that over- and underflow,
    N.L == 0, the cone's edge, penumbrae, zero and non-unit dirW, intensities 0, negative, 1e30 and inf — every third record
    with a NaN, zero or non-unit normal: the fused query equals the composed loop bit for bit, clampUpper FLT_MAX and 1, both
    materials"""
    nan = F("nan")
    normals = [(nan, 0, 1), (0, 0, 0), (-0.0, 0.0, -0.0), (0, 3.5, 0), (nan, nan, nan), (F("inf"), 0, 0)]
    cases = 0
    for count in (1, 3, 4):
        desc, keep = er.two_triangle_scene(pkg.abi, count)
        ctx = pkg.Context(0)
        ctx.set_scene(desc)
        for c in er.light_cases():
            if len(c.lights) != count:
                continue
            ctx.set_lights(list(er.make_lights(pkg.abi, c.lights)))
            rng = np.random.default_rng(cases)
            rec = rr.with_view(c.surf, rng)
            for j, i in enumerate(range(1, len(rec), 3)):
                if j % 2:
                    rec[i, 4:7] = np.array(normals[(j // 2) % len(normals)], F)
            seeds = rng.integers(0, 2**32, len(rec), dtype=np.uint64).astype(U)
            for mat, clamp in ((1, FLT_MAX), (0, 1.0), (1, 1.0), (0, FLT_MAX)):
                got = ris_query(ctx, rec, seeds, 4, 2, mat, clamp=clamp)
                want = rr.ris_compose(DeviceBackend(ctx, mat), rec, seeds, 4, 2, clamp=clamp, min_t=MIN_T)
                _assert_same(got, want, f"{c.name} mat {mat} clamp {clamp}")
                if clamp == 1.0:
                    assert not (got["color"][:, 0:3] > 4.0).any()
            cases += 1
        torch.cuda.synchronize()
        ctx.close()
    assert cases > 3


class _Room(dr.DirectScene):
    def __init__(self, pkg, lights=None):
        super().__init__(pkg, lights)
        self._pkg = pkg

    def camera(self, aspect):
        cam = self._pkg.abi.Camera()
        v3 = lambda *v: (C.c_float * 3)(*v)  # noqa: E731
        assert self._pkg.load_library().bdpt_camera_look_at(v3(0.3, 0.2, 3.4), v3(0.0, -0.1, 0.0), v3(0.0, 1.0, 0.0), 24.0, 24.0, aspect, 1.0,
                                                            C.byref(cam)) == 0
        return cam


@pytest.mark.parametrize("mat", [1, 0])
def test_execute_equals_the_query_and_tiles_reproduce_the_frame(pkg, mat):
    """(5) bdpt_ris_execute on a 64 x 48 G-buffer of the room with three lights equals the query fed that G-buffer (seeds
    initRand(pixel, frameCount), V from the camera); two row tiles write only their rows, with the whole frame's values;
    background pixels get (diffuse, 1); GGX without a camera is BDPT_E_STATE"""
    from test_gpu_sky_mis import _gbuffer_records
    sc = _Room(pkg, dr.gr.three_lights(pkg.abi))
    pipe = pkg.FramePipeline(sc, W, H, max_depth=3, min_t=MIN_T)
    ctx, st = pipe.ctx, pipe._stream_ptr()
    ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, st)
    torch.cuda.synchronize()
    M, K = 4, 2
    images = {}
    for frame in (0, 0, 5):
        pipe.ris_frame = frame
        img = host(pipe.ris_lighting(M, K, mat_index=mat, use_hints=frame == 5)).copy()
        p = pipe.last_ris_params
        assert pipe.ris_frame == frame + 1 and (p.frameCount, p.matIndex, p.candidates, p.samples) == (frame, mat, M, K)
        if frame in images:
            assert np.array_equal(bits(img), bits(images[frame]))
        images[frame] = img
    assert not np.array_equal(bits(images[0]), bits(images[5]))
    for frame, img in images.items():
        rec, seeds = _gbuffer_records(pipe, frame, mat)
        got = ris_query(ctx, rec, seeds, M, K, mat)
        assert np.array_equal(bits(img), bits(got["color"].reshape(H, W, 4))), frame
        background = rec.view(np.int32)[:, 23] < 0
        assert background.any() and (got["color"][~background, 0:3] > 0).any()
        assert np.array_equal(bits(img.reshape(-1, 4)[background, 0:3]), bits(rec[background, 12:15]))
    for y0, y1 in ((0, 16), (16, H)):
        tile = pkg.Context(0)
        tile.set_scene(sc.desc)
        tile.resize(W, H, y0, y1, 3)
        out = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
        if mat == 0:
            with pytest.raises(pkg.BdptError, match="no camera"):
                tile.ris_execute(pipe.gb, out, candidates=M, samples=K, mat_index=0, min_t=MIN_T, stream=st)
            tile.set_camera(pipe.cam)
        tile.ris_execute(pipe.gb, out, candidates=M, samples=K, mat_index=mat, min_t=MIN_T, stream=st)
        torch.cuda.synchronize()
        got = host(out)
        assert np.array_equal(bits(got[y0:y1]), bits(images[0][y0:y1])), (y0, y1)
        rows = np.ones(H, bool)
        rows[y0:y1] = False
        assert (got[rows] == -7.0).all()
        tile.close()
    torch.cuda.synchronize()
    pipe.close()


def test_captured_query(pkg, ob):
    """(6) one ris_lighting call captured: exactly one kernel node, capturing allocates nothing; two replays with different
    seeds in the same tensor each equal the eager call.  The first area-lights call inside a capture on an unprepared context
    returns BDPT_E_STATE and enqueues nothing."""
    from test_gpu_ao import _captured_once
    s = _scene(pkg, ob, "sixteen")
    ctx, rec, n = s["ctx"], s["rec"], len(s["rec"])
    M, K, mat = 8, 2, 0
    surf, sd = gpu(rec), gpu(s["seeds"].view(np.int32))
    outs = dict(color=torch.zeros((n, 4), dtype=torch.float32, device="cuda"), seeds_out=torch.zeros(n, dtype=torch.int32, device="cuda"),
                traced=torch.zeros(n, dtype=torch.int32, device="cuda"), reservoirs=torch.zeros((n, K, 4), dtype=torch.int32, device="cuda"))

    def enqueue(st):
        ctx.ris_lighting(surf, sd, M, K, mat_index=mat, use_hints=True, min_t=MIN_T, out=outs["color"], seeds_out=outs["seeds_out"],
                         traced=outs["traced"], reservoirs=outs["reservoirs"], stream=st)

    eager = _captured_once(enqueue, outs, [0])
    want = ris_query(ctx, rec, s["seeds"], M, K, mat, hints=True)
    _assert_same({k: host(v) if v.dtype == torch.float32 else host(v).view(U) for k, v in eager.items()}, want, "eager")
    # a graph of the call, replayed after the seeds changed in place
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        st = C.c_void_p(side.cuda_stream)
        graph = torch.cuda.CUDAGraph()
        graph.capture_begin()
        enqueue(st)
        graph.capture_end()
        for shift in (1, 2):
            other = (s["seeds"] * U(2654435761) + U(shift)).astype(U)
            sd.copy_(gpu(other.view(np.int32)))
            graph.replay()
            side.synchronize()
            got = {k: host(v) if v.dtype == torch.float32 else host(v).view(U) for k, v in outs.items()}
            _assert_same(got, ris_query(ctx, rec, other, M, K, mat, hints=True), f"replay {shift}")
        # an unprepared context: the emitter table cannot be built inside a capture
        fresh = pkg.Context(0)
        fresh.set_scene(s["scene"].desc)
        probe = torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda")
        pad = torch.zeros(1, device="cuda")
        g2 = torch.cuda.CUDAGraph()
        g2.capture_begin()
        pad.add_(1)
        with pytest.raises(pkg.BdptError, match="before stream capture") as refused:
            fresh.ris_lighting(surf, sd, M, K, area_lights=True, out=probe, stream=st)
        assert "-2" in str(refused.value) or "STATE" in str(refused.value)  # BDPT_E_STATE
        g2.capture_end()
        g2.replay()
        side.synchronize()
        assert (host(probe) == -7.0).all()
        del graph, g2
    torch.cuda.synchronize()
    fresh.close()


def test_error_cases_through_the_c_abi(pkg, ob):
    """(7) every error case in the documented order, nothing enqueued"""
    a = pkg.abi
    lib = pkg.load_library()
    s = _scene(pkg, ob, "three")
    ctx = pkg.Context(0)
    n = 256
    surf = torch.zeros((n, 24), dtype=torch.float32, device="cuda")
    seeds = torch.zeros(n, dtype=torch.int32, device="cuda")
    alive = torch.ones(n, dtype=torch.uint8, device="cuda")
    cnt = torch.full((4,), n, dtype=torch.int32, device="cuda")
    col = torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda")
    outs = {k: torch.full((n * 8,), -7, dtype=torch.int32, device="cuda") for k in ("so", "tr", "rs")}
    img = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
    gpos = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    gh = torch.zeros((3, H, W, 4), dtype=torch.float16, device="cuda")
    P = dict(sf=surf.data_ptr(), sd=seeds.data_ptr(), b=alive.data_ptr(), n=cnt.data_ptr(), col=col.data_ptr(), img=img.data_ptr(),
             gp=gpos.data_ptr(), gn=gh[0].data_ptr(), gd=gh[1].data_ptr(), gs=gh[2].data_ptr(), **{k: t.data_ptr() for k, t in outs.items()})

    def q(h=ctx._h, num=n, M=4, K=2, mat=0, cnt=None, flags=0, reserved=0, clamp=10.0, sf=P["sf"], sd=P["sd"], al=None, color=P["col"], so=None,
          tr=None, rs=None, desc=True):
        d = a.RisDesc()
        d.num, d.flags, d.numDevice, d.matIndex, d.candidates, d.samples, d.clampUpper, d.minT, d.reserved = num, flags, cnt, mat, M, K, clamp, 1e-4, reserved
        d.surfaces, d.alive, d.seeds, d.color, d.seedsOut, d.traced, d.reservoirs = sf, al, sd, color, so, tr, rs
        return lib.bdpt_ris_query(h, C.byref(d) if desc else None, None)

    def x(h=ctx._h, M=4, K=2, mat=0, flags=0, reserved=0, clamp=10.0, gp=P["gp"], gn=P["gn"], gd=P["gd"], gs=P["gs"], out=P["img"], params=True,
          gbuffer=True):
        p = a.RisParams(0, clamp, 1e-4, M, K, mat, flags, reserved)
        gb = a.GBuffer()
        gb.worldPosition, gb.worldNormal, gb.materialDiffuse, gb.materialSpecRough = gp, gn, gd, gs
        return lib.bdpt_ris_execute(h, C.byref(p) if params else None, C.byref(gb) if gbuffer else None, out, None)

    err = lambda: lib.bdpt_last_error(ctx._h)  # noqa: E731
    assert q() == -2 and b"ris_query" in err() and b"no scene" in err()
    assert x() == -2 and b"ris_execute" in err()
    assert q(M=0) == -2  # the state comes first
    ctx.set_scene(s["scene"].desc)
    assert x() == -2 and b"no size" in err()
    ctx.resize(W, H, 0, H, 3)
    assert x() == -2 and b"no camera" in err() and x(M=0) == -2  # matIndex 0 reads V from the camera: state before arguments
    assert x(mat=1, M=0) == -1  # the Lambertian pass needs none
    ctx.set_camera(_Room(pkg).camera(W / H))
    nan = float("nan")
    bad = [
        q(h=None), q(desc=False), q(M=0), q(M=33), q(M=2**31), q(K=0), q(K=65), q(mat=2), q(flags=2), q(flags=4096 | 8), q(reserved=1),
        q(clamp=-1.0), q(clamp=nan), q(num=0, M=0), q(num=0, clamp=nan), q(sf=None), q(sf=P["sf"] + 4), q(sd=None), q(sd=P["sd"] + 2),
        q(color=None), q(color=P["col"] + 8), q(so=P["so"] + 2), q(tr=P["tr"] + 1), q(rs=P["rs"] + 8), q(cnt=P["n"] + 2),
        x(h=None), x(params=False), x(gbuffer=False), x(M=0), x(M=33), x(K=0), x(K=65), x(mat=2), x(flags=2), x(reserved=1), x(clamp=-1.0),
        x(clamp=nan), x(gp=None), x(gp=P["gp"] + 8), x(gn=None), x(gn=P["gn"] + 4), x(gd=None), x(gd=P["gd"] + 4), x(gs=None),
        x(gs=P["gs"] + 4), x(out=None), x(out=P["img"] + 8),
    ]
    assert all(rc == -1 for rc in bad), bad
    assert q(num=0, sf=None, sd=None, color=None) == 0
    torch.cuda.synchronize()
    for t in list(outs.values()) + [col, img]:
        assert (host(t) == -7).all()
    # and the good calls: every record at the origin with N = 0 has N.L = 0: nothing is selected, colour 0 after its draws; a
    # zero worldPosition.w is the background, which takes the (zero) diffuse
    assert q(al=P["b"], so=P["so"], tr=P["tr"], rs=P["rs"], cnt=P["n"], flags=4097) == 0 and q(mat=1) == 0 and x() == 0
    assert x(mat=1, gs=None, flags=1) == 0  # the Lambertian pass does not read MaterialSpecRough
    torch.cuda.synchronize()
    assert (host(col) == np.array([0, 0, 0, 1], F)).all() and (host(outs["tr"])[:n] == 0).all()
    state = np.zeros(1, U)
    for _ in range(16):
        state = rr.next_rand(state)[0]
    assert (host(outs["so"])[:n].view(U) == state[0]).all()
    assert (host(outs["rs"]).view(U).reshape(-1, 4)[:n * 2, 0] == rr.NO_LIGHT).all()
    assert (host(img) == np.array([0, 0, 0, 1], F)).all()
    ctx.close()


def test_cpp_host_pass_equals_the_python_pipeline(pkg, tmp_path):
    """(8) bdpt_render --ris 4 --ris-samples 2 --raw on the Cornell box at 64 x 36, frame 0, equals FramePipeline.ris_lighting(4, 2):
    Lambertian, GGX with hints, and Lambertian with the emitter table"""
    import __graft_entry__ as ge
    exe = os.path.join(ge.PKG_DIR, "host", "bdpt_render")
    assert os.path.exists(exe), "host/bdpt_render not built (run __graft_entry__.build())"
    w, h = 64, 36
    scene = pkg.Scene.cornell()
    pipe = pkg.FramePipeline(scene, w, h)
    pipe.ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, pipe._stream_ptr())
    images = []
    for extra, kw in (([], dict(mat_index=1)), (["--ris-ggx", "--ris-hints"], dict(mat_index=0, use_hints=True)),
                      (["--area-lights", "--ris-clamp", "2.5"], dict(mat_index=1, area_lights=True, clamp=2.5))):
        raw = tmp_path / f"ris{len(images)}.f32"
        r = subprocess.run([exe, "--scene", "cornell", "--width", str(w), "--height", str(h), "--frames", "1", "--ris", "4", "--ris-samples", "2"] +
                           extra + ["--out", str(tmp_path / "ris.pfm"), "--raw", str(raw)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "resampled direct lighting" in r.stdout, r.stdout + r.stderr
        cpp = np.fromfile(raw, F).reshape(h, w, 4)
        pipe.ris_frame = 0
        img = host(pipe.ris_lighting(4, 2, **kw)).copy()
        p = pipe.last_ris_params
        assert (p.frameCount, p.candidates, p.samples) == (0, 4, 2)
        assert np.array_equal(bits(cpp), bits(img)), extra
        assert (cpp[..., 3] == 1.0).all() and (cpp[..., 0:3] > 0).any()
        images.append(cpp)
    assert not np.array_equal(bits(images[0]), bits(images[1])) and not np.array_equal(bits(images[0]), bits(images[2]))
    pipe.close()
    scene.close()
