"""GPU tests of reservoir reuse (csrc/reuse.hip): bdpt_reuse_query and bdpt_reuse_execute against the definition,
reuse_reference.reuse_compose, over the CPU oracle and over the composed device loop the call replaces — per source
prev(state) -> Context.sample_lights -> clamp, the selected sample again at every neighbour, then Context.trace_rays("any") —
and bdpt_ris_execute_reservoirs against bdpt_ris_execute and bdpt_ris_query.  Every comparison is on words viewed as integers,
over every item; two NaNs count as equal."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library is loaded, as test_gpu_gi.py explains)

import direct_reference as dr
import edge_records as er
import reuse_reference as ur
import ris_reference as rr
from area_scenes import AreaScene, bits
from test_gpu_ris import H, MIN_T, W, DeviceBackend, _assert_same, _Room, _scene, ris_query
from walk_loop import gpu, host

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
FLT_MAX = rr.FLT_MAX
OUTPUTS = ("color", "seeds_out", "traced", "out")
NONE = ur.NONE


def reuse_query(ctx, rec, seeds, res_in, nbr=None, pool=None, mat=1, area=False, alive=None, count=None, fill=-7, **kw):
    """one bdpt_reuse_query with every optional output -> dict of numpy arrays; pool: (records, reservoirs, alive or None);
    fill: what the outputs hold before"""
    n = len(rec)
    col = torch.full((n, 4), float(fill), dtype=torch.float32, device="cuda")
    so, trc = (torch.full((n,), int(fill), dtype=torch.int32, device="cuda") for _ in range(2))
    ro = torch.full((n, 4), int(fill), dtype=torch.int32, device="cuda")
    extra = {}
    if pool is not None:
        extra = dict(pool_surfaces=gpu(pool[0]), pool_reservoirs=gpu(np.ascontiguousarray(pool[1]).view(np.int32)),
                     pool_alive=None if pool[2] is None else gpu(pool[2]))
    res = ctx.reuse_lighting(gpu(rec), gpu(np.ascontiguousarray(seeds).view(np.int32)), gpu(np.ascontiguousarray(res_in).view(np.int32)),
                             neighbor_index=None if nbr is None else gpu(np.ascontiguousarray(nbr).view(np.int32)), mat_index=mat,
                             area_lights=area, min_t=MIN_T, alive=None if alive is None else gpu(alive), out=col, seeds_out=so, traced=trc,
                             reservoirs_out=ro, count=count, **extra, **kw)
    assert res is col
    torch.cuda.synchronize()
    return dict(color=host(col), seeds_out=host(so).view(U), traced=host(trc).view(U), out=host(ro).view(U))


def compose(backend, rec, seeds, res_in, lights_count, nbr=None, pool=None, alive=None, **kw):
    extra = {} if pool is None else dict(pool_rec=pool[0], pool_res=pool[1], pool_alive=pool[2])
    return ur.reuse_compose(backend, rec, seeds, res_in, lights_count, neighbor_index=nbr, alive=alive, **extra, **kw)


def _neighbors(rng, n, pool_num, k):
    """k random pool entries per item; every fifth slot names none, every seventh an index past the pool"""
    nbr = rng.integers(0, pool_num, (n, k), dtype=np.uint64).astype(U)
    flat = nbr.reshape(-1)
    flat[::5] = NONE
    flat[3::7] = U(pool_num) + (np.arange(len(flat[3::7])) % 3).astype(U) * U(2**30)
    return nbr


def _first_stage(ctx, rec, seeds, M, mat, area=False):
    return ris_query(ctx, rec, (seeds * U(747796405) + U(12345)).astype(U), M, 1, mat, area=area)["reservoirs"][:, 0, :].copy()


@pytest.mark.parametrize("mat", [1, 0])
@pytest.mark.parametrize("name", ["room", "three", "sixteen"])
def test_equals_the_oracle_and_the_loop(pkg, ob, name, mat):
    """(1) 1, 3 and 16 lights; 3,064 items with 64 miss records and a run of 256 dead items in the middle.  Inputs from a real
    bdpt_ris_query with 4 candidates (inM = poolM = 4).  neighbors 8 over the items themselves without rejection; neighbors 3
    over the previous reuse's records (their M words) with the normal and plane tests on and maxM biting; neighbors 1 over a
    distinct pool; neighbors 0.  color, seeds_out, traced and out equal reuse_compose over the oracle and over the device
    queries; skipped slots, empty records and selections from a neighbour all occur."""
    s = _scene(pkg, ob, name)
    ctx, rec, seeds = s["ctx"], s["rec"], s["seeds"]
    n, L = len(rec), len(s["lights"])
    oracle = rr.OracleBackend(ob, pkg.abi, s["lib"], s["osc"], s["lights"], mat, MIN_T)
    loop = DeviceBackend(ctx, mat)
    rng = np.random.default_rng(77)
    first = _first_stage(ctx, rec, seeds, 4, mat)
    seen = dict(skipped=0, empty=0, neighbour=0)

    def check(what, res_in, nbr, pool=None, with_loop=True, **kw):
        got = reuse_query(ctx, rec, seeds, res_in, nbr, pool, mat, **kw)
        want = compose(oracle, rec, seeds, res_in, L, nbr, pool, **kw)
        _assert_same(got, want, f"{name} mat {mat} {what}: the oracle", outputs=OUTPUTS)
        if with_loop:
            _assert_same(got, compose(loop, rec, seeds, res_in, L, nbr, pool, **kw), f"{name} mat {mat} {what}: the loop", outputs=OUTPUTS)
        lv = want["live"]
        assert (got["traced"][~lv] == 0).all() and np.array_equal(got["seeds_out"][~lv], seeds[~lv])
        assert np.array_equal(bits(got["color"][~lv, 0:3]), bits(rec[~lv, 12:15])) and (got["color"][:, 3] == 1.0).all()
        assert (got["out"][~lv] == np.array([rr.NO_LIGHT, 0, 0, 0], U)).all()
        status = got["out"][lv, 0] >> U(16)
        assert np.array_equal(got["traced"][lv], status & U(1))
        seen["skipped"] += int(want["skipped"].sum())
        seen["empty"] += int(want["empty"].sum())
        seen["neighbour"] += int((want["source"] > 0).sum())
        return got

    a = check("8 neighbours", first, _neighbors(rng, n, n, 8), in_m=4, pool_m=4)
    status = a["out"][:, 0] >> U(16)
    assert (status == rr.STATUS_RAY).any() and (status == (rr.STATUS_RAY | rr.STATUS_OCCLUDED)).any()  # lit and shadowed
    assert (a["out"][:, 3] > 4).any() and (a["out"][:, 3] <= 36).all()
    b = check("3 neighbours of a previous reuse", a["out"], _neighbors(rng, n, n, 3), normal_min=0.5, plane_max=0.75, max_m=6,
              with_loop=name == "three")
    assert (b["out"][:, 3] <= a["out"][:, 3].max() + 18).all()
    other = rng.permutation(n)[:1500]
    pool = (np.ascontiguousarray(rec[other]), np.ascontiguousarray(a["out"][other]), (np.arange(1500) % 11 != 3).astype(np.uint8))
    check("1 neighbour of a distinct pool", first, _neighbors(rng, n, 1500, 1), pool, in_m=4, with_loop=name == "sixteen")
    check("no neighbour", first, None, in_m=4, with_loop=False)
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("mat", [1, 0])
def test_emitter_table_samples_are_reused(pkg, ob, mat):
    """(2) the Cornell box with its emissive patch, a textured and an alpha-masked emitter and four lights: first stage and
    reuse with area_lights; equal to the composed loop for both materials and, for the Lambertian one, to the oracle
    composition; some item ends with a table sample that came from a neighbour"""
    cornell = pkg.Scene.cornell()
    sc = AreaScene(pkg, cornell, point_light=True, relit=True)
    pipe = pkg.FramePipeline(sc, W, H, max_depth=3, min_t=MIN_T)
    ctx = pipe.ctx
    rays = pipe.camera_rays()
    hits = torch.empty((W * H, 4), dtype=torch.float32, device="cuda")
    pipe.trace_rays(rays, "closest", out=hits)
    rec = host(pipe.shade_hits(rays, hits, normal_map=False))[::2].copy()
    torch.cuda.synchronize()
    n = len(rec)
    rng = np.random.default_rng(5)
    seeds = rng.integers(0, 2**32, n, dtype=np.uint64).astype(U)
    nl = int(sc.desc.numLights)
    first = _first_stage(ctx, rec, seeds, 4, mat, area=True)
    nbr = np.stack([(np.arange(n) + d) % n for d in (1, n - 1, 32, 7)], axis=1).astype(U)
    got = reuse_query(ctx, rec, seeds, first, nbr, None, mat, area=True, in_m=4, pool_m=4, normal_min=0.5)
    want = compose(DeviceBackend(ctx, mat, area=True), rec, seeds, first, nl + 1, nbr, in_m=4, pool_m=4, normal_min=0.5)
    _assert_same(got, want, f"area mat {mat}: the loop", outputs=OUTPUTS)
    if mat == 1:
        lib = ob.load_oracle(pkg.abi)
        osc = lib.oracle_scene_create(C.byref(sc.desc))
        lights = (pkg.abi.Light * nl)(*[sc.desc.lights[i] for i in range(nl)])
        oracle = rr.OracleBackend(ob, pkg.abi, lib, osc, lights, 1, MIN_T, area=True)
        assert oracle.table
        _assert_same(got, compose(oracle, rec, seeds, first, nl + 1, nbr, in_m=4, pool_m=4, normal_min=0.5), "area: the oracle", outputs=OUTPUTS)
        lib.oracle_scene_destroy(osc)
    light = got["out"][:, 0] & U(0xFFFF)
    assert ((light == nl) & (want["source"] > 0)).any() and (light < nl).any() and (light[light != rr.NO_LIGHT] <= nl).all()
    torch.cuda.synchronize()
    pipe.close()
    cornell.close()


def test_hostile_records_give_the_defined_words(pkg, ob):
    """(3) own and pool records with light ids at and past the light count and 0xffff, W NaN, +-inf, negative and -0, M 0 and
    0xffffffff (read from the records), neighbour indices at and past the pool: the call equals the definition over the oracle,
    and every item none of whose sources was touched gives what it gave before"""
    s = _scene(pkg, ob, "three")
    ctx, rec, seeds = s["ctx"], s["rec"], s["seeds"]
    n, L = len(rec), 3
    rng = np.random.default_rng(9)
    oracle = rr.OracleBackend(ob, pkg.abi, s["lib"], s["osc"], s["lights"], 1, MIN_T)
    clean = reuse_query(ctx, rec, seeds, _first_stage(ctx, rec, seeds, 4, 1), _neighbors(rng, n, n, 2), in_m=4, pool_m=4)["out"]
    nbr = _neighbors(rng, n, n, 3)
    base = reuse_query(ctx, rec, seeds, clean, nbr)
    bad = clean.copy()
    touched = np.zeros(n, bool)
    touched[rng.choice(n, 600, replace=False)] = True
    t = np.nonzero(touched)[0]
    words = [("light", v) for v in (3, 4, 100, 0xFFFF, 0xFFFE)] + \
            [("W", v) for v in (np.nan, np.inf, -np.inf, -1.0, -0.0, 1e38, 1e-45)] + [("M", v) for v in (0, 0xFFFFFFFF, 1 << 24, (1 << 24) + 1)]
    for j, i in enumerate(t):
        kind, v = words[j % len(words)]
        if kind == "light":
            bad[i, 0] = (bad[i, 0] & U(0xFFFF0000)) | U(v)
        elif kind == "W":
            bad[i, 2] = np.array([v], F).view(U)[0]
        else:
            bad[i, 3] = U(v)
    got = reuse_query(ctx, rec, seeds, bad, nbr)
    want = compose(oracle, rec, seeds, bad, L, nbr)
    _assert_same(got, want, "hostile records", outputs=OUTPUTS)
    ok = nbr < n
    beside = ~touched & ~(ok & touched[np.where(ok, nbr, 0)]).any(axis=1)
    assert beside.sum() > 500 and (~beside).sum() > 600
    _assert_same(got, base, "the items beside the hostile records", keep=beside, outputs=OUTPUTS)
    assert (got["out"][:, 3] <= 4 * (1 << 24)).all() and (got["out"][:, 3] > (1 << 24)).any()


def test_edge_records_beside_ordinary_ones(pkg):
    """(4) edge_records.light_cases — a point at the light, distances that over- and underflow, N.L == 0, the cone's edge,
    intensities 0, negative, 1e30 and inf — every third record with a NaN, zero or non-unit normal, as test_gpu_ris.py builds
    them: first stage and reuse over two neighbours equal the composed loop bit for bit, clampUpper FLT_MAX and 1, both
    materials, with the rejection tests on (a NaN normal skips the slot)"""
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
            n = len(rec)
            seeds = rng.integers(0, 2**32, n, dtype=np.uint64).astype(U)
            nbr = np.stack([(np.arange(n) + 1) % n, (np.arange(n) + n // 2) % n], axis=1).astype(U)
            for mat, clamp in ((1, FLT_MAX), (0, 1.0)):
                first = ris_query(ctx, rec, (seeds + U(1)).astype(U), 4, 1, mat, clamp=clamp)["reservoirs"][:, 0, :].copy()
                kw = dict(in_m=4, pool_m=4, clamp=clamp, normal_min=-1.0, plane_max=1e30)
                got = reuse_query(ctx, rec, seeds, first, nbr, None, mat, **kw)
                want = compose(DeviceBackend(ctx, mat), rec, seeds, first, count, nbr, **kw)
                _assert_same(got, want, f"{c.name} mat {mat} clamp {clamp}", outputs=OUTPUTS)
            cases += 1
        torch.cuda.synchronize()
        ctx.close()
    assert cases > 3


def test_item_counts_device_counts_and_alive(pkg, ob):
    """(5) a device count below the capacity leaves the outputs beyond it untouched; 0, 1, 63, 64 and 65 items; alive masks on
    the items and on the pool; seeds_out in place; host arrays"""
    s = _scene(pkg, ob, "three")
    ctx, rec, seeds = s["ctx"], s["rec"], s["seeds"]
    n, L = len(rec), 3
    oracle = rr.OracleBackend(ob, pkg.abi, s["lib"], s["osc"], s["lights"], 1, MIN_T)
    first = _first_stage(ctx, rec, seeds, 4, 1)
    nbr = _neighbors(np.random.default_rng(3), n, n, 2)
    kw = dict(in_m=4, pool_m=4)
    want = compose(oracle, rec, seeds, first, L, nbr, **kw)
    for m in (1, 63, 64, 65):
        small = np.where(nbr[:m] < m, nbr[:m], NONE).astype(U)
        _assert_same(reuse_query(ctx, rec[:m], seeds[:m], first[:m], small, **kw), compose(oracle, rec[:m], seeds[:m], first[:m], L, small, **kw),
                     f"{m} items", outputs=OUTPUTS)
    empty = ctx.reuse_lighting(gpu(rec[:0]), gpu(seeds[:0].view(np.int32)), gpu(first[:0].view(np.int32)))
    assert tuple(empty.shape) == (0, 4)
    for m in (0, 1, 65, 1000, n, n + 9):
        cnt = torch.tensor([m], dtype=torch.int32, device="cuda")
        got = reuse_query(ctx, rec, seeds, first, nbr, count=cnt, **kw)
        k = min(m, n)
        _assert_same({x: got[x][:k] for x in OUTPUTS}, {x: want[x][:k] for x in OUTPUTS}, f"device count {m}", outputs=OUTPUTS)
        assert (got["color"][k:] == -7.0).all() and all((got[x].view(np.int32)[k:] == -7).all() for x in OUTPUTS[1:]), m
    for alive in ((np.arange(n) % 3 != 1).astype(np.uint8), np.zeros(n, np.uint8)):
        got = reuse_query(ctx, rec, seeds, first, nbr, alive=alive, **kw)  # (the pool is the items: its alive bytes are theirs)
        _assert_same(got, compose(oracle, rec, seeds, first, L, nbr, alive=alive, **kw), "alive", outputs=OUTPUTS)
        dead = alive == 0
        assert np.array_equal(bits(got["color"][dead, 0:3]), bits(rec[dead, 12:15])) and np.array_equal(got["seeds_out"][dead], seeds[dead])
        assert (got["out"][dead] == np.array([rr.NO_LIGHT, 0, 0, 0], U)).all()
    st = gpu(seeds.view(np.int32))
    ctx.reuse_lighting(gpu(rec), st, gpu(first.view(np.int32)), neighbor_index=gpu(nbr.view(np.int32)), seeds_out=st, min_t=MIN_T, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(host(st).view(U), want["seeds_out"])
    h = ctx.reuse_lighting(rec[:65], seeds[:65], first[:65], in_m=4, min_t=MIN_T)
    assert isinstance(h, np.ndarray) and dr.same_bits(h, compose(oracle, rec[:65], seeds[:65], first[:65], L, None, in_m=4)["color"]).all()


def _pixel_query(ctx, rec, seeds, res_in, nbr, pool_res, mat, **kw):
    """the query fed a frame's pixels: the pool is the frame itself with pool_res"""
    return reuse_query(ctx, rec, seeds, res_in, nbr, (rec, pool_res, None), mat, **kw)


@pytest.mark.parametrize("mat", [1, 0])
def test_execute_equals_the_query_and_tiles_reproduce_the_frame(pkg, mat):
    """(6) on a 64 x 48 G-buffer of the room with three lights: bdpt_ris_execute_reservoirs writes bdpt_ris_execute's colour
    and, at geometry pixels, bdpt_ris_query's records (a background pixel's are left alone); bdpt_reuse_execute equals the
    query fed the same pixels — seeds initRand(initRand(pixel, frame), 0x52455553) — for a caller's neighbour image, the same
    pixel of another pool, and offsets drawn within a radius of 5; two row tiles write only their rows, with the frame's values"""
    from test_gpu_sky_mis import _gbuffer_records
    sc = _Room(pkg, dr.gr.three_lights(pkg.abi))
    pipe = pkg.FramePipeline(sc, W, H, max_depth=3, min_t=MIN_T)
    ctx, st = pipe.ctx, pipe._stream_ptr()
    ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, st)
    torch.cuda.synchronize()
    M, frame = 4, 3
    rec, seeds = _gbuffer_records(pipe, frame, mat)
    alive = rec.view(np.int32)[:, 23] >= 0
    assert alive.any() and (~alive).any()
    img = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
    plain = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
    rsv = torch.full((H, W, 2, 4), -7, dtype=torch.int32, device="cuda")
    ctx.ris_execute(pipe.gb, plain, candidates=M, samples=2, mat_index=mat, min_t=MIN_T, frame_count=frame, stream=st)
    ctx.ris_execute(pipe.gb, img, candidates=M, samples=2, mat_index=mat, min_t=MIN_T, frame_count=frame, reservoirs=rsv, stream=st)
    torch.cuda.synchronize()
    q = ris_query(ctx, rec, seeds, M, 2, mat)
    assert np.array_equal(bits(host(img)), bits(host(plain))) and np.array_equal(bits(host(img).reshape(-1, 4)), bits(q["color"]))
    got_rsv = host(rsv).view(U).reshape(-1, 2, 4)
    assert np.array_equal(got_rsv[alive], q["reservoirs"][alive]) and (got_rsv[~alive].view(np.int32) == -7).all()
    # the reuse stage: own records are sample 0 of the first stage, the pool's those of another frame
    first = np.ascontiguousarray(q["reservoirs"][:, 0, :])
    first[~alive] = U(0xDEAD)  # nothing reads a background pixel's record
    other = np.ascontiguousarray(ris_query(ctx, rec, _gbuffer_records(pipe, frame + 1, mat)[1], M, 1, mat)["reservoirs"][:, 0, :])
    forked = ur.fork_seeds(np.arange(W * H), frame)
    rng = np.random.default_rng(4)
    image = _neighbors(rng, W * H, W * H, 3)
    drawn, after = ur.drawn_neighbors(forked, W, H, 4, 5)
    cam = tuple(float(v) for v in pipe.cam.posW)
    kw = dict(in_m=M, pool_m=M, max_m=6, normal_min=0.5, plane_max=0.5)
    cases = {
        "image": (dict(neighbors=3, neighbor_index=gpu(image.view(np.int32).reshape(H, W, 3))), forked, image, first),
        "same pixel": (dict(neighbors=1, same_pixel=True, pool_reservoirs=gpu(other.view(np.int32).reshape(H, W, 4))), forked,
                       np.arange(W * H, dtype=U)[:, None], other),
        "drawn": (dict(neighbors=4, radius=5), after, drawn, first),
    }
    tiles = []
    for y0, y1 in ((0, 16), (16, H)):
        tile = pkg.Context(0)
        tile.set_scene(sc.desc)
        tile.resize(W, H, y0, y1, 3)
        tile.set_camera(pipe.cam)
        tiles.append((tile, y0, y1))
    for what, (args, s0, nbr, pool_res) in cases.items():
        want = _pixel_query(ctx, rec, s0, first, nbr, pool_res, mat, **kw)
        assert (want["traced"] > 0).any()
        col = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
        ro = torch.full((H, W, 4), -7, dtype=torch.int32, device="cuda")
        ctx.reuse_execute(pipe.gb, col, gpu(first.view(np.int32).reshape(H, W, 4)), mat_index=mat, min_t=MIN_T, frame_count=frame,
                          pool_camera_pos=cam, reservoirs_out=ro, stream=st, **args, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(bits(host(col).reshape(-1, 4)), bits(want["color"])), what
        assert np.array_equal(host(ro).view(U).reshape(-1, 4), want["out"]), what
        col2 = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
        ro2 = torch.full((H, W, 4), -7, dtype=torch.int32, device="cuda")
        for tile, y0, y1 in tiles:
            before = host(col2).copy()
            tile.reuse_execute(pipe.gb, col2, gpu(first.view(np.int32).reshape(H, W, 4)), mat_index=mat, min_t=MIN_T, frame_count=frame,
                               pool_camera_pos=cam, reservoirs_out=ro2, stream=st, **args, **kw)
            torch.cuda.synchronize()
            rows = np.ones(H, bool)
            rows[y0:y1] = False
            assert np.array_equal(bits(host(col2)[rows]), bits(before[rows])), (what, y0)
        assert np.array_equal(bits(host(col2)), bits(host(col))) and np.array_equal(host(ro2), host(ro)), what
    if mat == 0:
        bare = pkg.Context(0)
        bare.set_scene(sc.desc)
        bare.resize(W, H, 0, H, 3)
        with pytest.raises(pkg.BdptError, match="no camera"):
            bare.reuse_execute(pipe.gb, img, gpu(first.view(np.int32).reshape(H, W, 4)), mat_index=0, stream=st)
        bare.close()
    for tile, _, _ in tiles:
        tile.close()
    torch.cuda.synchronize()
    pipe.close()


def _look_from(pkg, eye, aspect):
    cam = pkg.abi.Camera()
    v3 = lambda *v: (C.c_float * 3)(*v)  # noqa: E731
    assert pkg.load_library().bdpt_camera_look_at(v3(*eye), v3(0.0, -0.1, 0.0), v3(0.0, 1.0, 0.0), 24.0, 24.0, aspect, 1.0, C.byref(cam)) == 0
    return cam


@pytest.mark.parametrize("spatial", [3, 0])
def test_restir_lighting_is_the_three_calls(pkg, spatial):
    """(7) FramePipeline.restir_lighting (GGX) over three frames, the camera moved and the G-buffer rendered anew before each,
    equals Context.ris_execute -> reuse_execute (same pixel of a hand-kept copy of last frame's reservoirs and G-buffer, seen
    from last frame's camera) -> reuse_execute (drawn offsets) made by hand; without a spatial pass the history's records are
    the first stage's on frame 1 (their count is the call's) and a reuse pass's after; the first frame has no history;
    set_lights drops it (tests/test_reuse_cpu.py has the geometry updates); bad arguments are refused before anything is allocated; a tile
    pipeline refuses"""
    sc = _Room(pkg, dr.gr.three_lights(pkg.abi))
    pipe = pkg.FramePipeline(sc, W, H, max_depth=3, min_t=MIN_T)
    ctx, st = pipe.ctx, pipe._stream_ptr()
    M, R = 4, 6
    for kw in (dict(candidates=0), dict(candidates=33), dict(candidates=M, max_m=0), dict(candidates=M, max_m=2.5), dict(candidates=M, spatial=9),
               dict(candidates=M, spatial=2, radius=0), dict(candidates=M, temporal=1), dict(candidates=M, mat_index=2)):
        with pytest.raises(pkg.BdptError):
            pipe.restir_lighting(**kw)
    assert pipe._restir is None and pkg.RESTIR_CHANNEL not in pipe.channels and pipe.restir_frame == 0
    mk = lambda: torch.zeros((H, W, 4), dtype=torch.int32, device="cuda")  # noqa: E731
    hist, a, b, c = mk(), mk(), mk(), mk()
    names = ("WorldPosition", "WorldNormal", "MaterialDiffuse", "MaterialSpecRough")
    kept = [torch.zeros_like(pipe.channels[n]) for n in names]
    kept_gb = pkg.abi.GBuffer(*([t.data_ptr() for t in kept] + [None, None]))
    col = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    images, hist_cam, hist_m = [], None, 0
    for frame, eye in enumerate(((0.3, 0.2, 3.4), (0.5, 0.25, 3.3), (0.1, 0.3, 3.2))):
        pipe.cam = _look_from(pkg, eye, W / H)
        ctx.set_camera(pipe.cam)
        ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, st)
        pipe.gbuffer_frame += 1
        cam = tuple(float(v) for v in pipe.cam.posW)
        got = host(pipe.restir_lighting(M, spatial=spatial, radius=R, temporal=True, mat_index=0)).copy()
        ctx.ris_execute(pipe.gb, col, candidates=M, mat_index=0, min_t=MIN_T, frame_count=frame, reservoirs=a.view(H, W, 1, 4), stream=st)
        cur, in_m = a, M
        if frame:
            ctx.reuse_execute(pipe.gb, col, a, neighbors=1, same_pixel=True, pool_gbuffer=kept_gb, pool_reservoirs=hist, pool_camera_pos=hist_cam,
                              in_m=M, pool_m=hist_m, max_m=20 * M, normal_min=0.9, mat_index=0, min_t=MIN_T, frame_count=2 * frame,
                              reservoirs_out=b, stream=st)
            cur, in_m = b, 0
        if spatial:
            ctx.reuse_execute(pipe.gb, col, cur, neighbors=spatial, radius=R, pool_camera_pos=cam, in_m=in_m, pool_m=in_m, max_m=20 * M,
                              normal_min=0.9, mat_index=0, min_t=MIN_T, frame_count=2 * frame + 1, reservoirs_out=c, stream=st)
            cur, in_m = c, 0
        hist.copy_(cur)
        for dst, n in zip(kept, names):
            dst.copy_(pipe.channels[n])
        hist_cam, hist_m = cam, in_m
        torch.cuda.synchronize()
        assert np.array_equal(bits(got), bits(host(col))), frame
        assert pipe.restir_frame == frame + 1 and pipe._restir["m"] == hist_m
        images.append(got)
    assert (images[2][..., 0:3] > 0).any() and not np.array_equal(bits(images[1]), bits(images[2]))
    assert pipe._restir["valid"]
    pipe.set_lights(list(sc.lights))
    assert not pipe._restir["valid"]
    pipe.close()
    tiled = pkg.FramePipeline(sc, W, H, max_depth=3, min_t=MIN_T, tile=(0, 16))
    with pytest.raises(pkg.BdptError, match="tile or stripes"):
        tiled.restir_lighting(M)
    tiled.close()


def test_cpp_host_pass_equals_the_python_pipeline_and_resumes(pkg, tmp_path):
    """(7b) bdpt_render --ris 4 --ris-spatial 3 --ris-radius 5 --ris-temporal --raw on the Cornell box at 64 x 36 over three
    frames (the G-buffer pass jitters the camera every frame, so the history's G-buffer copy differs from the frame's) equals
    FramePipeline.restir_lighting's third image: Lambertian; GGX with the emitter table, a clamp and --ris-max-m; temporal
    reuse alone.  Two frames, a checkpoint, and one resumed frame equal the uninterrupted run; a checkpoint is refused under
    other settings."""
    import os
    import subprocess
    import __graft_entry__ as ge
    exe = os.path.join(ge.PKG_DIR, "host", "bdpt_render")
    assert os.path.exists(exe), "host/bdpt_render not built (run __graft_entry__.build())"
    w, h = 64, 36
    scene = pkg.Scene.cornell()
    base = [exe, "--scene", "cornell", "--width", str(w), "--height", str(h), "--out", str(tmp_path / "o.pfm")]

    def render(extra, frames, raw, more=()):
        r = subprocess.run(base + ["--frames", str(frames), "--raw", str(raw)] + extra + list(more), capture_output=True, text=True, timeout=300)
        return r

    images = []
    for k, (extra, kw) in enumerate((
            (["--ris", "4", "--ris-spatial", "3", "--ris-radius", "5", "--ris-temporal"], dict(spatial=3, radius=5, temporal=True)),
            (["--ris", "4", "--ris-spatial", "2", "--ris-temporal", "--ris-ggx", "--area-lights", "--ris-clamp", "2.5", "--ris-max-m", "12"],
             dict(spatial=2, temporal=True, mat_index=0, area_lights=True, clamp=2.5, max_m=12)),
            (["--ris", "4", "--ris-temporal"], dict(temporal=True)))):
        raw = tmp_path / f"restir{k}.f32"
        r = render(extra, 3, raw)
        assert r.returncode == 0 and "ReSTIR direct lighting" in r.stdout, r.stdout + r.stderr
        cpp = np.fromfile(raw, F).reshape(h, w, 4)
        pipe = pkg.FramePipeline(scene, w, h)
        for _ in range(3):
            pipe.ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, pipe._stream_ptr())
            pipe.gbuffer_frame += 1
            img = host(pipe.restir_lighting(4, **kw)).copy()
        assert np.array_equal(bits(cpp), bits(img)), extra
        assert (cpp[..., 3] == 1.0).all() and (cpp[..., 0:3] > 0).any()
        pipe.close()
        images.append(cpp)
        # two frames, a checkpoint, one resumed frame
        ck = tmp_path / f"restir{k}.ckpt"
        r = render(extra, 2, tmp_path / "part.f32", ["--checkpoint", str(ck)])
        assert r.returncode == 0 and os.path.exists(ck), r.stderr
        r = render(extra, 1, tmp_path / "resumed.f32", ["--resume", str(ck)])
        assert r.returncode == 0, r.stderr
        assert np.array_equal(bits(np.fromfile(tmp_path / "resumed.f32", F)), bits(cpp.reshape(-1))), extra
        assert not np.array_equal(bits(np.fromfile(tmp_path / "part.f32", F)), bits(cpp.reshape(-1)))
    assert not np.array_equal(bits(images[0]), bits(images[2]))
    for other in (["--ris", "5", "--ris-temporal"], ["--ris", "4", "--ris-temporal", "--ris-max-m", "7"], ["--ris", "4", "--ris-temporal", "--ris-spatial", "1"],
                  ["--ris", "4"]):
        r = render(other, 1, tmp_path / "no.f32", ["--resume", str(tmp_path / "restir2.ckpt")])
        assert r.returncode != 0 and "cannot resume" in r.stderr, (other, r.stderr)
    scene.close()


def test_captured_query(pkg, ob):
    """(8) one reuse_lighting call captured: exactly one kernel node, capturing allocates nothing; two replays with different
    seeds in the same tensor each equal the eager call"""
    from test_gpu_ao import _captured_once
    s = _scene(pkg, ob, "sixteen")
    ctx, rec, n = s["ctx"], s["rec"], len(s["rec"])
    mat = 0
    first = _first_stage(ctx, rec, s["seeds"], 4, mat)
    nbr = _neighbors(np.random.default_rng(2), n, n, 3)
    surf, sd, rin, ni = gpu(rec), gpu(s["seeds"].view(np.int32)), gpu(first.view(np.int32)), gpu(nbr.view(np.int32))
    outs = dict(color=torch.zeros((n, 4), dtype=torch.float32, device="cuda"), seeds_out=torch.zeros(n, dtype=torch.int32, device="cuda"),
                traced=torch.zeros(n, dtype=torch.int32, device="cuda"), out=torch.zeros((n, 4), dtype=torch.int32, device="cuda"))

    def enqueue(st):
        ctx.reuse_lighting(surf, sd, rin, neighbor_index=ni, in_m=4, pool_m=4, mat_index=mat, min_t=MIN_T, out=outs["color"],
                           seeds_out=outs["seeds_out"], traced=outs["traced"], reservoirs_out=outs["out"], stream=st)

    as_np = lambda d: {k: host(v) if v.dtype == torch.float32 else host(v).view(U) for k, v in d.items()}  # noqa: E731
    eager = _captured_once(enqueue, outs, [0])
    _assert_same(as_np(eager), reuse_query(ctx, rec, s["seeds"], first, nbr, None, mat, in_m=4, pool_m=4), "eager", outputs=OUTPUTS)
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
            _assert_same(as_np(outs), reuse_query(ctx, rec, other, first, nbr, None, mat, in_m=4, pool_m=4), f"replay {shift}", outputs=OUTPUTS)
        del graph
    torch.cuda.synchronize()


def test_error_cases_through_the_c_abi(pkg, ob):
    """(9) every error case in the documented order, the aliasing refusals among them; nothing enqueued"""
    a = pkg.abi
    lib = pkg.load_library()
    s = _scene(pkg, ob, "three")
    ctx = pkg.Context(0)
    n = 256
    surf = torch.zeros((n, 24), dtype=torch.float32, device="cuda")
    words = {k: torch.zeros(n * 4, dtype=torch.int32, device="cuda") for k in ("sd", "rin", "pool", "nbr")}
    col = torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda")
    outs = {k: torch.full((n * 4,), -7, dtype=torch.int32, device="cuda") for k in ("so", "tr", "ro")}
    img = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
    frame = {k: torch.zeros((H, W, 4), dtype=torch.int32, device="cuda") for k in ("fin", "fpool", "fnbr")}
    fout = torch.full((H, W, 4), -7, dtype=torch.int32, device="cuda")
    gpos = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    gh = torch.zeros((3, H, W, 4), dtype=torch.float16, device="cuda")
    P = dict(sf=surf.data_ptr(), col=col.data_ptr(), img=img.data_ptr(), fout=fout.data_ptr(), gp=gpos.data_ptr(), gn=gh[0].data_ptr(),
             gd=gh[1].data_ptr(), gs=gh[2].data_ptr(), **{k: t.data_ptr() for d in (words, outs, frame) for k, t in d.items()})

    def q(h=ctx._h, num=n, K=2, mat=0, flags=0, reserved=(0, 0), clamp=10.0, sf=P["sf"], sd=P["sd"], rin=P["rin"], ps=P["sf"], pool=P["pool"],
          nbr=P["nbr"], pn=n, color=P["col"], so=None, tr=None, ro=None, desc=True):
        d = a.ReuseDesc()
        d.num, d.flags, d.matIndex, d.neighbors, d.maxM, d.poolNum, d.clampUpper, d.minT = num, flags, mat, K, 8, pn, clamp, 1e-4
        d.normalMin, d.planeMax, d.reserved = -1.0, 1e30, (C.c_uint32 * 2)(*reserved)
        d.surfaces, d.seeds, d.poolSurfaces, d.pool, d.neighborIndex, d.color, d.seedsOut, d.traced, d.out = sf, sd, ps, pool, nbr, color, so, tr, ro
        setattr(d, "in", rin)
        return lib.bdpt_reuse_query(h, C.byref(d) if desc else None, None)

    pool_gb = a.GBuffer()
    pool_gb.worldPosition, pool_gb.worldNormal, pool_gb.materialDiffuse, pool_gb.materialSpecRough = P["gp"], P["gn"], P["gd"], P["gs"]

    def x(h=ctx._h, K=1, mat=0, flags=1, radius=0, reserved=0, clamp=10.0, gp=P["gp"], out=P["img"], fin=P["fin"], pool=P["fpool"], nbr=None,
          ro=None, pgb=pool_gb, params=True, gbuffer=True):
        p = a.ReuseParams()
        p.clampUpper, p.minT, p.matIndex, p.flags, p.neighbors, p.radius, p.maxM, p.reserved = clamp, 1e-4, mat, flags, K, radius, 8, reserved
        p.normalMin, p.planeMax = -1.0, 1e30
        p.poolGbuffer, p.pool, p.neighborIndex, p.outReservoirs = (C.pointer(pgb) if pgb is not None else None), pool, nbr, ro
        setattr(p, "in", fin)
        gb = a.GBuffer()
        gb.worldPosition, gb.worldNormal, gb.materialDiffuse, gb.materialSpecRough = gp, P["gn"], P["gd"], P["gs"]
        return lib.bdpt_reuse_execute(h, C.byref(p) if params else None, C.byref(gb) if gbuffer else None, out, None)

    err = lambda: lib.bdpt_last_error(ctx._h)  # noqa: E731
    assert q() == -2 and b"reuse_query" in err() and b"no scene" in err()
    assert x() == -2 and b"reuse_execute" in err()
    assert q(K=9) == -2  # the state comes first
    ctx.set_scene(s["scene"].desc)
    assert x() == -2 and b"no size" in err()
    ctx.resize(W, H, 0, H, 3)
    assert x() == -2 and b"no camera" in err() and x(K=9) == -2  # matIndex 0 reads V from the camera: state before arguments
    assert x(mat=1, K=9) == -1  # the Lambertian pass needs none
    ctx.set_camera(_Room(pkg).camera(W / H))
    nan = float("nan")
    bad = [
        q(h=None), q(desc=False), q(K=9), q(K=2**31), q(mat=2), q(flags=1), q(flags=4096 | 8), q(reserved=(1, 0)), q(reserved=(0, 1)),
        q(clamp=-1.0), q(clamp=nan), q(num=0, K=9), q(num=0, clamp=nan), q(sf=None), q(sf=P["sf"] + 4), q(sd=None), q(sd=P["sd"] + 2),
        q(rin=None), q(rin=P["rin"] + 8), q(ps=None), q(ps=P["sf"] + 8), q(pool=None), q(pool=P["pool"] + 4), q(nbr=None), q(nbr=P["nbr"] + 1),
        q(color=None), q(color=P["col"] + 8), q(so=P["so"] + 2), q(tr=P["tr"] + 1), q(ro=P["ro"] + 8),
        q(ro=P["rin"]), q(ro=P["pool"]), q(ro=P["rin"], K=0),  # out aliases in or pool
        x(h=None), x(params=False), x(gbuffer=False), x(K=9), x(mat=2), x(flags=2), x(flags=3), x(reserved=1), x(clamp=-1.0), x(clamp=nan),
        x(K=2), x(K=0), x(nbr=P["fnbr"]),  # SAME_PIXEL goes with one neighbour and no image
        x(flags=0, K=2), x(flags=0, K=2, radius=1025),  # drawn offsets need a radius
        x(gp=None), x(gp=P["gp"] + 8), x(out=None), x(out=P["img"] + 8), x(fin=None), x(fin=P["fin"] + 4), x(pool=None), x(pgb=None),
        x(flags=0, K=2, nbr=P["fnbr"] + 2), x(ro=P["fout"] + 8), x(ro=P["fin"]), x(ro=P["fpool"]),
    ]
    assert all(rc == -1 for rc in bad), bad
    assert q(num=0, sf=None, sd=None, rin=None, color=None) == 0
    torch.cuda.synchronize()
    for t in list(outs.values()) + [col, img, fout]:
        assert (host(t) == -7).all()
    # and the good calls: empty records select nothing: colour 0 after the draws, the counts add up; a zero worldPosition.w is
    # the background, which takes the (zero) diffuse
    assert q(so=P["so"], tr=P["tr"], ro=P["ro"], flags=4096) == 0 and q(K=0, ps=None, pool=None, nbr=None) == 0 and q(pn=0, ps=None, pool=None) == 0
    assert x(ro=P["fout"]) == 0 and x(flags=0, K=3, radius=2) == 0 and x(flags=0, K=0, pool=None, pgb=None) == 0
    assert x(flags=0, K=2, nbr=P["fnbr"], mat=1) == 0
    torch.cuda.synchronize()
    assert (host(col) == np.array([0, 0, 0, 1], F)).all() and (host(outs["tr"])[:n] == 0).all()
    state = np.zeros(1, U)
    for _ in range(3):
        state = rr.next_rand(state)[0]
    assert (host(outs["so"])[:n].view(U) == state[0]).all()
    assert (host(outs["ro"]).view(U).reshape(-1, 4)[:n] == np.array([rr.NO_LIGHT, 0, 0, 0], U)).all()  # the records' M words are 0
    assert (host(img) == np.array([0, 0, 0, 1], F)).all() and (host(fout).view(U) == np.array([rr.NO_LIGHT, 0, 0, 0], U)).all()
    ctx.close()
