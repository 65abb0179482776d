"""GPU tests of the light queries (csrc/light_query.hip): bdpt_light_query in its NEE and EMIT modes.  Every comparison is
bit for bit, on the float words viewed as integers, and every yardstick is bdpt_execute, the CPU oracle or an existing
hook: the composed calls (emit -> sample_lights -> trace_rays, with sample_bsdf / shade_hits for deeper vertices) must
reproduce the pass's NEE-only frame (NO_SPLAT | NO_CONNECT), per-item results must equal oracle_area_light_sample and
bdpt_test_area_light_sample, and the analytic lights a float32 numpy restatement built from oracle_rng and oracle_sincos2pi."""
import ctypes as C

import numpy as np
import pytest

from area_scenes import (AREA, LCG_INV, NEE_TOP_DRAW_STATES, NO_CONNECT, NO_SPLAT, AreaScene, DescArrays, bits, emitter_soup,
                         oracle_sample, states_for_top_draw)

pytestmark = pytest.mark.gpu

F = np.float32
LCG_A, LCG_C = 1664525, 1013904223


def _gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _lcg(s):
    """the state after one nextRand and the float it returns"""
    s1 = ((s.astype(np.uint64) * LCG_A + LCG_C) % (1 << 32)).astype(np.uint32)
    return s1, (s1 & np.uint32(0xFFFFFF)).astype(F) / F(0x01000000)


def _lcg_back(s1):
    """the state one nextRand before s1"""
    x = (s1.astype(np.uint64) + ((1 << 32) - LCG_C)) % (1 << 32)
    return ((x * LCG_INV) % (1 << 32)).astype(np.uint32)


def _pixel_states(ctx, n, frame_count):
    """initRand(pix, frameCount) of pixels 0 .. n-1: bdpt_test_rng gives the state after the first draw; one LCG step back"""
    st, _ = ctx.test_rng(np.arange(n, dtype=np.uint32), np.full(n, frame_count & 0xFFFFFFFF, np.uint32), 1)
    return _lcg_back(st[:, 0])


def _normalize(v):
    inv = F(1.0) / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    return v * inv[:, None]


def _clamp_vec(v, hi):
    """clampVec (MaterialUtils.hlsli:15-18) as device_math.hpp has it: NaN -> +0"""
    y = np.where(v > 0, v, F(0))
    return np.where(y < hi, y, F(hi)).astype(F)


def _surfaces_from_gbuffer(pipe):
    """bdpt_surface records of eye vertex 1 as initPathsLane builds it from the G-buffer channels: half values widened,
    linearRoughness = the spec-rough w, V = normalize(camPos - pos) in float32, prim 0 where worldPosition.w != 0 else -1"""
    n = pipe.W * pipe.H
    wp = _np(pipe.channels["WorldPosition"]).reshape(n, 4)
    ch = {k: _np(pipe.channels[k].float()).reshape(n, 4) for k in ("WorldNormal", "MaterialDiffuse", "MaterialSpecRough", "Emissive")}
    valid = wp[:, 3] != 0
    cam = np.array(pipe.cam.posW[:], F)
    surf = np.zeros((n, 24), F)
    surf[:, 0:3] = wp[:, 0:3]
    surf[:, 4:7] = ch["WorldNormal"][:, 0:3]
    surf[:, 7] = ch["MaterialSpecRough"][:, 3]
    with np.errstate(all="ignore"):
        surf[:, 8:11] = _normalize(cam[None] - wp[:, 0:3])
    surf[:, 12:15] = ch["MaterialDiffuse"][:, 0:3]
    surf[:, 16:19] = ch["MaterialSpecRough"][:, 0:3]
    surf[:, 20:23] = ch["Emissive"][:, 0:3]
    surf[~valid] = 0
    surf.view(np.int32)[:, 23] = np.where(valid, 0, -1)
    return surf, valid, ch["MaterialDiffuse"], ch["Emissive"]


def _start_image(valid, dif, emis):
    """what init_paths leaves in `out` (oracle bdptPixel :59-66, :155-158): the background colour with w 1, else the cleared
    pixel plus its emissive where any component is positive"""
    n = len(valid)
    out = np.zeros((n, 4), F)
    em = valid & (emis[:, 0:3] > 0).any(axis=1)
    out[em] = F(0) + emis[em]
    out[~valid, 0:3] = dif[~valid, 0:3]
    out[~valid, 3] = F(1)
    return out


def _add_term(out, valid, color, value, visible, k, hi):
    """out += clampVec((cameraPath[t].color * direct) / k) where the light is visible, w += 1 (oracle :1287-1300)"""
    with np.errstate(all="ignore"):
        shade = _clamp_vec((color * value) / F(k), hi)
    shade = np.where((visible & valid)[:, None], shade, F(0))
    out[:, 0:3] = np.where(valid[:, None], out[:, 0:3] + shade, out[:, 0:3])
    out[:, 3] = np.where(valid, out[:, 3] + F(1), out[:, 3])
    return shade


def _status(rec):
    w = rec.view(np.uint32)[:, 11]
    return w & 0xFFFF, w >> 16  # light, status


def _nee_term(pipe, surf_t, seeds_t, compacted):
    """One NEE term through the queries: (record (N, 12), visible (N,) bool, chained seeds, rays traced).  compacted: with
    occluder hints and the dense ray list traced by its device count; else every item's ray is traced and masked by status."""
    import torch
    n = surf_t.shape[0]
    chain = torch.empty(n, dtype=torch.int32, device="cuda")
    if not compacted:
        rec = pipe.sample_lights(surf_t, seeds_t, seeds_out=chain)
        vis = pipe.trace_rays(rec[:, 0:8].contiguous(), "any")
        torch.cuda.synchronize()
        r = _np(rec)
        _, status = _status(r)
        assert (status <= 1).all()  # no hints asked for
        return r, (_np(vis) != 0) & (status == 1), chain, n
    cr = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    ci = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    cc = torch.zeros(1, dtype=torch.int32, device="cuda")
    cv = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    rec = pipe.sample_lights(surf_t, seeds_t, use_hints=True, seeds_out=chain, compact=(cr, ci, cc))
    pipe.trace_rays(cr, "any", out=cv, count=cc)
    torch.cuda.synchronize()
    r, k = _np(rec), int(cc.item())
    _, status = _status(r)
    items = _np(ci)[:k]
    assert np.array_equal(np.sort(items), np.nonzero(status == 1)[0])  # exactly the items worth a ray, each once
    assert (_np(ci)[k:] == -1).all() and (_np(cv)[k:] == 7).all()
    assert np.array_equal(bits(_np(cr)[:k]), bits(r[items, 0:8]))  # and their rays
    visible = np.zeros(n, bool)
    visible[items] = _np(cv)[:k] != 0
    return r, visible, chain, k


_CORNELL = {}


def _scene(pkg, which):
    if which == "cornell":
        if "base" not in _CORNELL:
            _CORNELL["base"] = pkg.Scene.cornell()
        return AreaScene(pkg, _CORNELL["base"], point_light=True, relit=True), 72, 56
    return pkg.Scene.atrium(1, 30000), 96, 54


_DEPTH1 = {}


def _depth1(pkg, which, mat, area):
    """The depth-1 NEE-only frame of the pass and its composition from the queries, both ways; cached per configuration."""
    import torch
    key = (which, mat, area)
    if key in _DEPTH1:
        return _DEPTH1[key]
    scene, W, H = _scene(pkg, which)
    pipe = pkg.FramePipeline(scene, W, H, max_depth=1, mat_index=mat, flags=NO_SPLAT | NO_CONNECT | (AREA if area else 0))
    n = W * H
    gp, p = pipe.render_frame()
    torch.cuda.synchronize()
    ref = _np(pipe.output).reshape(n, 4).copy()
    cnt = pipe.ctx.counters().as_dict()
    surf, valid, dif, emis = _surfaces_from_gbuffer(pipe)
    seed0 = _gpu(_pixel_states(pipe.ctx, n, p.frameCount))
    seedL = torch.empty(n, dtype=torch.int32, device="cuda")
    emit = pipe.emit_lights(seed0, seeds_out=seedL)
    res = dict(ref=ref, counters=cnt, valid=valid, emit=_np(emit), numLights=int(scene.desc.numLights),
               info=pipe.ctx.area_light_info() if area else None)
    hi = F(p.clampUpper)
    for compacted in (False, True):
        rec, visible, _, traced = _nee_term(pipe, _gpu(surf), seedL, compacted)
        out = _start_image(valid, dif, emis)
        shade = _add_term(out, valid, np.ones((n, 3), F), rec[:, 8:11], visible, 2, hi)
        res["compact" if compacted else "plain"] = dict(out=out, rec=rec, traced=traced, shade_if_visible=shade)
    # (shade of the compacted run, before visibility: what the pass tests for "worth a ray")
    with np.errstate(all="ignore"):
        res["clamped"] = _clamp_vec(res["compact"]["rec"][:, 8:11] / F(2), hi)
    pipe.close()
    if which != "cornell":
        scene.close()
    _DEPTH1[key] = res
    return res


CONFIGS = [(w, m, a) for w in ("cornell", "atrium") for m in (0, 1) for a in (False, True)]


@pytest.mark.parametrize("which,mat,area", CONFIGS)
def test_composed_depth1_frame_equals_the_pass(pkg, which, mat, area):
    """emit_lights (seedL) -> sample_lights on the G-buffer's eye vertex -> trace_rays(any) -> emissive + clampVec(value / 2)
    where visible equals bdpt_execute(maxDepth 1, NO_SPLAT | NO_CONNECT) in all four words of every pixel, with per-item
    rays and with hints + the compacted list; the two ways give the same records but for the hint bit."""
    r = _depth1(pkg, which, mat, area)
    n = len(r["valid"])
    assert 0 < r["valid"].sum() <= n
    for way in ("plain", "compact"):
        diff = (bits(r[way]["out"]) != bits(r["ref"])).any(axis=1)
        assert not diff.any(), f"{way}: {int(diff.sum())} of {n} pixels differ, first {int(np.argmax(diff))}"
    a, b = r["plain"]["rec"].view(np.uint32).copy(), r["compact"]["rec"].view(np.uint32).copy()
    b[:, 11] &= ~np.uint32(2 << 16)
    assert np.array_equal(a, b)
    light, _ = _status(r["plain"]["rec"])
    lights_count = r["numLights"] + (1 if area and r["info"].totalWeight > 0 else 0)
    assert light[r["valid"]].max() == lights_count - 1  # every light is drawn, the table included
    assert (r["plain"]["rec"][~r["valid"]].view(np.uint32) == 0).all()
    if area:
        assert r["info"].numEmitters > 0 and (light == r["numLights"]).sum() > 0


@pytest.mark.parametrize("which,mat,area", CONFIGS)
def test_ray_economy(pkg, which, mat, area):
    """USE_HINTS + compaction on the depth-1 frame: the compacted count is the pass's raysNee plus the items whose value is
    non-zero but whose clampVec(value / 2) is all zero (the pass tests the clamped term, the query the value: these are
    values without a positive component, NaN where dot(N, V) <= 0 under GGX, for which the query tries no hint, as the pass
    tries none), and the items the hint answered are the pass's hintedNee."""
    r = _depth1(pkg, which, mat, area)
    _, status = _status(r["compact"]["rec"])
    extra = int(((status == 1) & (r["clamped"] == 0).all(axis=1)).sum())
    print(f"{which} mat {mat} area {area}: compacted {r['compact']['traced']}, raysNee {r['counters']['raysNee']}, "
          f"extra {extra}, hinted {int((status & 2 != 0).sum())}, hintedNee {r['counters']['hintedNee']}, items {len(status)}")
    assert r["compact"]["traced"] == r["counters"]["raysNee"] + extra
    assert int((status & 2 != 0).sum()) == r["counters"]["hintedNee"]
    assert r["compact"]["traced"] < r["plain"]["traced"]


@pytest.mark.parametrize("mat", [0, 1])
def test_composed_depth3_nee_frame_equals_the_pass(pkg, mat):
    """maxDepth 3 on the Cornell AreaScene with the table on: eye vertices 2 and 3 from sample_bsdf (the pixel's initRand
    state by value) -> trace_rays(closest, tmin = minT) -> shade_hits without the normal map, the colour the running
    product, term t with the chained seedsOut of term t - 1.  A miss follows the oracle's shootRay and bdptPixel
    :1231-1300: the payload keeps the previous geometry with colour 0 (a ghost vertex, which still gets its NEE term with
    the previous vertex's throughput), the walk stops, later vertices do not exist (records with prim -1: they only take
    their draw).  All pixels are compared."""
    import torch
    D = 3
    scene, W, H = _scene(pkg, "cornell")
    pipe = pkg.FramePipeline(scene, W, H, max_depth=D, mat_index=mat, flags=NO_SPLAT | NO_CONNECT | AREA)
    n = W * H
    gp, p = pipe.render_frame()
    torch.cuda.synchronize()
    ref = _np(pipe.output).reshape(n, 4).copy()
    surf, valid, dif, emis = _surfaces_from_gbuffer(pipe)
    seed0 = _gpu(_pixel_states(pipe.ctx, n, p.frameCount))
    seedL = torch.empty(n, dtype=torch.int32, device="cuda")
    pipe.emit_lights(seed0, seeds_out=seedL)
    # the eye walk
    vertex = {1: surf}
    color = {0: np.ones((n, 3), F)}
    payload = np.zeros((n, 24), F)  # initPayload: posW = the origin, the rest 0
    payload[:, 0:3] = surf[:, 0:3]
    s = _np(pipe.sample_bsdf(_gpu(surf), seed0))
    pcolor, L = s[:, 4:7].copy(), s[:, 0:3].copy()
    color[1] = pcolor.copy()
    alive = valid.copy()
    for depth in range(1, D):
        rays = np.zeros((n, 8), F)
        rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = payload[:, 0:3], F(pipe.min_t), L, F(1e38)
        rays[~alive] = 0
        rt = _gpu(rays)
        hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        pipe.trace_rays(rt, "closest", out=hits)
        new = pipe.shade_hits(rt, hits, normal_map=False)
        smp = _np(pipe.sample_bsdf(new, seed0))
        new = _np(new)
        hit = alive & (new.view(np.int32)[:, 23] >= 0)
        payload = np.where(hit[:, None], new, payload)
        with np.errstate(all="ignore"):
            pcolor = np.where(hit[:, None], pcolor * smp[:, 4:7], F(0)).astype(F)
        L = np.where(hit[:, None], smp[:, 0:3], L)
        v = payload.copy()
        v.view(np.int32)[:, 23] = np.where(alive, np.maximum(v.view(np.int32)[:, 23], 0), -1)  # ghost: computed; none: -1
        v[~alive, 0:23] = 0
        vertex[depth + 1], color[depth + 1] = v, pcolor.copy()
        print(f"mat {mat} bounce {depth}: {int(alive.sum())} rays, {int(hit.sum())} hits, {int((alive & ~hit).sum())} ghost vertices")
        alive = hit
    out = _start_image(valid, dif, emis)
    seeds = seedL
    hi = F(p.clampUpper)
    terms = 0
    for t in range(D):
        rec, visible, seeds, _ = _nee_term(pipe, _gpu(vertex[t + 1]), seeds, compacted=(t % 2 == 1))
        shade = _add_term(out, valid, color[t], rec[:, 8:11], visible, t + 2, hi)
        terms += int((shade != 0).any(axis=1).sum())
    assert terms > 0
    diff = (bits(out) != bits(ref)).any(axis=1)
    assert not diff.any(), f"{int(diff.sum())} of {n} pixels differ, first {int(np.argmax(diff))}"
    pipe.close()


def _lambert_value(lights_count, L, intensity, N, dif):
    """directIfVisible<false> (device_math.hpp) in its operation order"""
    d = (N[:, 0] * L[:, 0] + N[:, 1] * L[:, 1]) + N[:, 2] * L[:, 2]
    y = np.where(d > 0, d, F(0))
    ldn = np.where(y < 1, y, F(1)).astype(F)
    return (((F(lights_count) * ldn)[:, None] * intensity) * dif) / F(3.14159265358979323846)


def _table_states(rng, k, lights_count, seed):
    """query states whose selection draw picks the table (the last of lights_count lights): random ones, the states whose
    draw is the largest below 1 (states_for_top_draw), and states before the NEE top-draw states (one LCG step back)"""
    s = rng.integers(0, 2 ** 32, 3 * k, dtype=np.uint64).astype(np.uint32)
    _, r = _lcg(s)
    s = s[np.minimum((r * F(lights_count)).astype(np.int32), lights_count - 1) == lights_count - 1][:k]
    back = _lcg_back(NEE_TOP_DRAW_STATES)
    _, rb = _lcg(back)
    back = back[np.minimum((rb * F(lights_count)).astype(np.int32), lights_count - 1) == lights_count - 1]
    return np.concatenate([s, states_for_top_draw(1024, seed), back])


def _table_parity(pkg, ob, ctx, desc, states, rng):
    lib = ob.load_oracle(pkg.abi)
    osc = lib.oracle_scene_create(C.byref(desc))
    n = len(states)
    after, _ = _lcg(states)  # the hooks take the state right after the selection draw
    # EMIT against mode 0
    so = _gpu(np.zeros(n, np.uint32).view(np.int32))
    em = _np(ctx.emit_lights(_gpu(states.view(np.int32)), min_t=0.125, area_lights=True, seeds_out=so))
    for name, ref in (("oracle", oracle_sample(lib, osc, 0, after)), ("hook", ctx.test_area_light_sample(0, after))):
        assert (ref.view(np.uint32)[:, 0] != 0).any() or n == 0
        assert np.array_equal(bits(em[:, 0:3]), bits(ref[:, 3:6])), name          # position
        assert np.array_equal(bits(em[:, 4:7]), bits(ref[:, 9:12])), name         # direction
        assert np.array_equal(bits(em[:, 8:11]), bits(ref[:, 12:15])), name       # colour
        assert np.array_equal(_np(so).view(np.uint32), ref.view(np.uint32)[:, 15]), name  # seedL
    assert (em[:, 3] == F(0.125)).all() and (em[:, 7] == F(1e38)).all() and (em.view(np.uint32)[:, 11] == 1).all()
    # NEE against mode 1: Lambertian records, so that the value is the intensity through three multiplications
    pts = rng.uniform(-5.0, 105.0, (n, 3)).astype(F)
    surf = np.zeros((n, 24), F)
    surf[:, 0:3] = pts
    nrm = rng.normal(size=(n, 3)).astype(F)
    surf[:, 4:7] = _normalize(nrm)
    surf[:, 12:15] = rng.uniform(0.1, 1.0, (n, 3)).astype(F)
    chain = _gpu(np.zeros(n, np.uint32).view(np.int32))
    rec = _np(ctx.sample_lights(_gpu(surf), _gpu(states.view(np.int32)), mat_index=1, min_t=0.125, area_lights=True, seeds_out=chain))
    assert np.array_equal(_np(chain).view(np.uint32), after)
    light, status = _status(rec)
    assert (light == 1).all()
    for name, ref in (("oracle", oracle_sample(lib, osc, 1, after, pts)), ("hook", ctx.test_area_light_sample(1, after, pts))):
        assert np.array_equal(bits(rec[:, 0:3]), bits(pts)) and (rec[:, 3] == F(0.125)).all()
        assert np.array_equal(bits(rec[:, 4:7]), bits(ref[:, 1:4])), name                           # L
        assert np.array_equal(bits(rec[:, 7]), bits(ref[:, 4] * (F(1.0) - F(1e-4)))), name          # d (1 - 1e-4)
        with np.errstate(all="ignore"):
            val = _lambert_value(2, ref[:, 1:4], ref[:, 5:8], surf[:, 4:7], surf[:, 12:15])
        assert np.array_equal(bits(rec[:, 8:11]), bits(val)), name
        assert np.array_equal(status, ((val != 0).any(axis=1)).astype(np.uint32)), name
    assert 0 < (status == 1).sum()
    # the GGX instance draws the same point: ray and distance are the Lambertian record's
    surf[:, 7] = rng.uniform(0.1, 1.0, n).astype(F)
    surf[:, 8:11] = _normalize(rng.normal(size=(n, 3)).astype(F))
    surf[:, 16:19] = rng.uniform(0.0, 1.0, (n, 3)).astype(F)
    ggx = _np(ctx.sample_lights(_gpu(surf), _gpu(states.view(np.int32)), mat_index=0, min_t=0.125, area_lights=True))
    assert np.array_equal(bits(ggx[:, 0:8]), bits(rec[:, 0:8]))
    lib.oracle_scene_destroy(osc)


@pytest.mark.parametrize("n", [65, 4097, 70000])
def test_table_items_match_oracle_and_hook(pkg, ob, n):
    """On emitter soups (tables that straddle a wave, a chunk of wave sums, and ~70 000 emitters), before and after a
    bdpt_update_geometry: NEE ray, distance and value equal oracle_area_light_sample / bdpt_test_area_light_sample mode 1
    (the value through a numpy restatement of lambertianDirect on their L and intensity), EMIT position, direction,
    colour and seedsOut equal mode 0.  The states all land on the table."""
    sc = emitter_soup(pkg, n, seed=n + 1)
    ctx = pkg.Context(0)
    ctx.set_scene(sc.desc)
    rng = np.random.default_rng(n)
    states = _table_states(rng, 200_000 if n == 70000 else 30_000, 2, n)
    _table_parity(pkg, ob, ctx, sc.desc, states, rng)
    P2 = (sc.P * F(1.7) - F(3.0)).astype(F)
    ctx.update_geometry(P2)
    moved = DescArrays(pkg.abi, P2, sc.N, sc.T, sc.I, sc.M, list(sc.mats), sc.textures, list(sc.lights))
    _table_parity(pkg, ob, ctx, moved.desc, states[::4], rng)
    ctx.close()


def _perpendicular(u):
    a = np.abs(u)
    xm = (((a[:, 0] - a[:, 1]) < 0) & ((a[:, 0] - a[:, 2]) < 0)).astype(np.uint32)
    ym = np.where((a[:, 1] - a[:, 2]) < 0, 1 ^ xm, 0).astype(np.uint32)
    zm = 1 ^ (xm | ym)
    return _cross(u, np.stack([xm, ym, zm], axis=1).astype(F))


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1).astype(F)


def _cos_hemisphere(lib, r0, r1, nrm):
    """getCosHemisphereSample (device_math.hpp) in float32, its sine and cosine from oracle_sincos2pi"""
    sn, cs = np.zeros_like(r1), np.zeros_like(r1)
    r1 = np.ascontiguousarray(r1, F)
    lib.oracle_sincos2pi(r1.ctypes.data, len(r1), sn.ctypes.data, cs.ctypes.data)
    bt = _perpendicular(nrm)
    tg = _cross(bt, nrm)
    r = np.sqrt(r0)
    z = np.sqrt(np.maximum(F(0), F(1) - r0))
    return ((tg * (r * cs)[:, None] + bt * (r * sn)[:, None]) + nrm * z[:, None]).astype(F)


def test_analytic_lights_in_emit(pkg, ob):
    """EMIT on the relit Cornell box (three point / spot lights and a directional one, no table): org and colour are the
    light's posW and intensity words; the direction equals an exact float32 numpy restatement of sampleUnitSphere and
    getCosHemisphereSample on oracle_rng's floats (sine and cosine from oracle_sincos2pi); seedsOut is the bdpt_test_rng
    state after 1 + 3 * rounds + 2 draws for a point or spot light (rounds: the rejection rounds of sampleUnitSphere) and
    after 1 + 2 draws for a directional light."""
    import torch
    lib = ob.load_oracle(pkg.abi)
    scene, _, _ = _scene(pkg, "cornell")
    ctx = pkg.Context(0)
    ctx.set_scene(scene.desc)
    n, draws, frame = 40000, 3 + 3 * 40, 0x1337
    st, fl = ctx.test_rng(np.arange(n, dtype=np.uint32), np.full(n, frame, np.uint32), draws)
    ost, ofl = np.zeros_like(st), np.zeros_like(fl)
    v0, v1 = np.arange(n, dtype=np.uint32), np.full(n, frame, np.uint32)
    lib.oracle_rng(v0.ctypes.data, v1.ctypes.data, n, draws, ost.ctypes.data, ofl.ctypes.data)
    assert np.array_equal(st, ost) and np.array_equal(bits(fl), bits(ofl))
    seed0 = _pixel_states(ctx, n, frame)
    so = torch.empty(n, dtype=torch.int32, device="cuda")
    em = _np(ctx.emit_lights(_gpu(seed0.view(np.int32)), min_t=0.5, seeds_out=so))
    so = _np(so).view(np.uint32)
    nl = int(scene.desc.numLights)
    index = np.minimum((ofl[:, 0] * F(nl)).astype(np.int32), nl - 1)
    assert np.array_equal(em.view(np.uint32)[:, 11], index.astype(np.uint32)) and set(index) == set(range(nl))
    lights = [scene.desc.lights[k] for k in range(nl)]
    pos = np.array([l.posW[:] for l in lights], F)[index]
    inten = np.array([l.intensity[:] for l in lights], F)[index]
    direc = np.array([l.dirW[:] for l in lights], F)[index]
    directional = np.array([l.type == pkg.abi.LIGHT_DIRECTIONAL for l in lights])[index]
    assert 0 < directional.sum() < n
    assert np.array_equal(bits(em[:, 0:3]), bits(pos)) and np.array_equal(bits(em[:, 8:11]), bits(inten))
    assert (em[:, 3] == F(0.5)).all() and (em[:, 7] == F(1e38)).all()
    # sampleUnitSphere: rounds of three draws until length(p) <= 1
    used = np.ones(n, np.int64)  # draws taken so far (the selection draw)
    axis = direc.copy()
    todo = ~directional
    rows = np.arange(n)
    while todo.any():
        assert (used[todo] + 5 <= draws).all()
        p = np.stack([ofl[rows, np.minimum(used + k, draws - 1)] * F(2.0) - F(1.0) for k in range(3)], axis=1).astype(F)
        ln = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
        axis[todo] = p[todo]
        used[todo] += 3
        todo = todo & (ln > F(1.0))
    d = _cos_hemisphere(lib, ofl[rows, used], ofl[rows, used + 1], axis)
    used += 2
    assert np.array_equal(bits(em[:, 4:7]), bits(d))
    assert np.array_equal(so, ost[rows, used - 1])
    assert (used[directional] == 3).all() and (used[~directional] >= 6).all() and ((used[~directional] - 3) % 3 == 0).all()
    ctx.close()


W, H = 96, 64


def _atrium_pipe(pkg, seed=2, area=True):
    scene = pkg.Scene.atrium(seed, 20000)
    pipe = pkg.FramePipeline(scene, W, H, max_depth=3, flags=AREA if area else 0)
    return scene, pipe


def _eye_surfaces(pipe):
    import torch
    rays = pipe.camera_rays()
    hits = torch.empty((W * H, 4), dtype=torch.float32, device="cuda")
    pipe.trace_rays(rays, "closest_cull_back", out=hits)
    return pipe.shade_hits(rays, hits)


def test_device_counts(pkg):
    """count = M < N: the first M items are written as without a count, later records, seeds and the compacted lists are
    left as they were, and the list holds items below M only."""
    import torch
    scene, pipe = _atrium_pipe(pkg)
    n = W * H
    surf = _eye_surfaces(pipe)
    seeds = _gpu((np.arange(n, dtype=np.uint32) * np.uint32(2654435761)).view(np.int32))
    full_nee, full_emit = pipe.sample_lights(surf, seeds, use_hints=True), pipe.emit_lights(seeds)
    full_so = torch.empty(n, dtype=torch.int32, device="cuda")
    pipe.emit_lights(seeds, seeds_out=full_so)
    torch.cuda.synchronize()
    _, status = _status(_np(full_nee))
    for m in (1000, 0, n + 5):
        cnt = torch.tensor([m], dtype=torch.int32, device="cuda")
        a = torch.full((n, 12), -7, dtype=torch.int32, device="cuda")
        e = torch.full((n, 12), -7, dtype=torch.int32, device="cuda")
        so = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        cr = torch.full((n, 8), -7.0, dtype=torch.float32, device="cuda")
        ci = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        cc = torch.zeros(1, dtype=torch.int32, device="cuda")
        pipe.sample_lights(surf, seeds, use_hints=True, out=a, compact=(cr, ci, cc), count=cnt)
        pipe.emit_lights(seeds, out=e, seeds_out=so, count=cnt.view(torch.uint32))
        torch.cuda.synchronize()
        k = min(m, n)
        for got, ref in ((a, full_nee), (e, full_emit)):
            g = _np(got).view(np.uint32)
            assert np.array_equal(g[:k], bits(_np(ref))[:k]) and (g[k:].view(np.int32) == -7).all()
        assert np.array_equal(_np(so)[:k], _np(full_so)[:k]) and (_np(so)[k:] == -7).all()
        kc = int(cc.item())
        assert kc == int((status[:k] == 1).sum())
        assert np.array_equal(np.sort(_np(ci)[:kc]), np.nonzero(status[:k] == 1)[0])
        assert (_np(ci)[kc:] == -7).all() and (_np(cr)[kc:] == -7.0).all()
    pipe.close()
    scene.close()


def test_after_a_device_update_on_the_same_stream(pkg, ob):
    """update_geometry, then the queries on one stream: EMIT and NEE samples of the table equal the oracle's on the moved
    scene (the update refreshed the emitter table on that stream), and differ from those before it."""
    import torch
    sc = emitter_soup(pkg, 3000, seed=5)
    ctx = pkg.Context(0)
    ctx.set_scene(sc.desc)
    ctx.prepare(pkg.abi.PREPARE_AREA_LIGHTS | pkg.abi.PREPARE_REFIT)
    rng = np.random.default_rng(12)
    states = _table_states(rng, 20000, 2, 3)
    n = len(states)
    after, _ = _lcg(states)
    pts = rng.uniform(0.0, 100.0, (n, 3)).astype(F)
    surf = np.zeros((n, 24), F)
    surf[:, 0:3], surf[:, 5], surf[:, 12:15] = pts, F(1), F(0.5)
    P2 = (sc.P * F(1.3) + F(2.0)).astype(F)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        st = C.c_void_p(side.cuda_stream)
        sg, tg, pg = _gpu(surf), _gpu(states.view(np.int32)), _gpu(P2)
        before = ctx.emit_lights(tg, area_lights=True, stream=st)
        ctx.update_geometry(pg, stream=st)
        em = ctx.emit_lights(tg, area_lights=True, stream=st)
        rec = ctx.sample_lights(sg, tg, mat_index=1, area_lights=True, stream=st)
    torch.cuda.synchronize()
    moved = DescArrays(pkg.abi, P2, sc.N, sc.T, sc.I, sc.M, list(sc.mats), sc.textures, list(sc.lights))
    lib = ob.load_oracle(pkg.abi)
    osc = lib.oracle_scene_create(C.byref(moved.desc))
    r0, r1 = oracle_sample(lib, osc, 0, after), oracle_sample(lib, osc, 1, after, pts)
    lib.oracle_scene_destroy(osc)
    em, rec = _np(em), _np(rec)
    assert np.array_equal(bits(em[:, 0:3]), bits(r0[:, 3:6])) and np.array_equal(bits(em[:, 8:11]), bits(r0[:, 12:15]))
    assert np.array_equal(bits(rec[:, 4:7]), bits(r1[:, 1:4]))
    assert not np.array_equal(bits(em[:, 0:3]), bits(_np(before)[:, 0:3]))  # the emitters did move
    ctx.close()


def test_frames_are_unchanged_by_the_queries(pkg):
    """frame, a burst of light queries, frame gives the image of two frames without them, bit for bit; counters and stage
    times the frame left are unchanged."""
    import torch
    scene = pkg.Scene.atrium(3, 20000)
    imgs = []
    for with_queries in (True, False):
        pipe = pkg.FramePipeline(scene, W, H, max_depth=4, flags=pkg.abi.PARAM_COUNTERS | AREA)
        pipe.ctx.enable_stage_timing(True)
        pipe.render_frame()
        if with_queries:
            torch.cuda.synchronize()
            before = pipe.ctx.counters().as_dict()
            times = pipe.ctx.stage_times()
            n = W * H
            surf = _eye_surfaces(pipe)
            seeds = _gpu(np.arange(n, dtype=np.int32))
            for hints in (False, True):
                cr = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
                ci = torch.zeros(n, dtype=torch.int32, device="cuda")
                cc = torch.zeros(1, dtype=torch.int32, device="cuda")
                pipe.sample_lights(surf, seeds, use_hints=hints, seeds_out=seeds, compact=(cr, ci, cc))
                pipe.trace_rays(cr, "any", count=cc)
                pipe.emit_lights(seeds, seeds_out=seeds)
                pipe.sample_lights(surf, seeds, use_hints=hints)
            torch.cuda.synchronize()
            assert pipe.ctx.counters().as_dict() == before
            assert pipe.ctx.stage_times() == times
        pipe.render_frame()
        torch.cuda.synchronize()
        imgs.append(_np(pipe.output))
        pipe.close()
    assert np.array_equal(imgs[0].view(np.uint32), imgs[1].view(np.uint32))
    scene.close()


def test_error_cases_through_the_c_abi(pkg):
    import torch
    a = pkg.abi
    lib = pkg.load_library()
    scene = pkg.Scene.cornell()
    ctx = pkg.Context(0)
    n = 256
    surf = torch.zeros((n, 24), dtype=torch.float32, device="cuda")
    surf.view(torch.int32)[:, 23] = -1
    seeds = torch.zeros(n, dtype=torch.int32, device="cuda")
    so = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    out = torch.full((n, 12), -7, dtype=torch.int32, device="cuda")
    cr = torch.full((n, 8), -7, dtype=torch.int32, device="cuda")
    ci = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    cc = torch.zeros(1, dtype=torch.int32, device="cuda")
    P = dict(s=surf.data_ptr(), sd=seeds.data_ptr(), so=so.data_ptr(), o=out.data_ptr(), cr=cr.data_ptr(), ci=ci.data_ptr(),
             cc=cc.data_ptr())

    def q(h=ctx._h, mode=a.LIGHT_NEE, num=n, cnt=None, mat=0, flags=0, s=P["s"], sd=P["sd"], so_=None, smp=P["o"], emt=None,
          comp=(None, None, None), desc=True):
        d = a.LightDesc()
        d.mode, d.num, d.numDevice, d.matIndex, d.flags, d.minT = mode, num, cnt, mat, flags, 1e-4
        d.surfaces, d.seeds, d.seedsOut, d.samples, d.emits = s, sd, so_, smp, emt
        d.compactRays, d.compactItems, d.compactCount = comp
        return lib.bdpt_light_query(h, C.byref(d) if desc else None, None)

    def e(**kw):
        kw.setdefault("smp", None)
        kw.setdefault("s", None)
        kw.setdefault("emt", P["o"])
        return q(mode=a.LIGHT_EMIT, **kw)

    full = (P["cr"], P["ci"], P["cc"])
    assert q() == -2 and e() == -2  # BDPT_E_STATE: no scene
    ctx.set_scene(scene.desc)
    bad = [
        q(h=None), q(desc=False), q(mode=2), q(mat=2), q(flags=2), q(flags=a.PARAM_AREA_LIGHTS << 1), q(s=None), q(s=P["s"] + 4),
        q(sd=None), q(sd=P["sd"] + 2), q(smp=None), q(smp=P["o"] + 8), q(so_=P["so"] + 1), q(cnt=P["sd"] + 2),
        q(comp=(P["cr"], None, None)), q(comp=(None, P["ci"], None)), q(comp=(None, None, P["cc"])), q(comp=(P["cr"], P["ci"], None)),
        q(comp=(P["cr"], None, P["cc"])), q(comp=(None, P["ci"], P["cc"])), q(comp=(P["cr"] + 8, P["ci"], P["cc"])),
        q(comp=(P["cr"], P["ci"] + 2, P["cc"])), q(comp=(P["cr"], P["ci"], P["cc"] + 1)),
        e(emt=None), e(emt=P["o"] + 4), e(sd=None), e(flags=a.LIGHT_USE_HINTS), e(comp=full), e(comp=(P["cr"], None, None)),
        e(so_=P["so"] + 2), e(cnt=P["sd"] + 1), e(mat=2),
        q(num=0, mode=2), q(num=0, comp=(P["cr"], None, None)),  # (found before the empty call returns)
    ]
    assert all(rc == -1 for rc in bad), bad
    assert q(num=0, s=None, sd=None, smp=None) == 0 and e(num=0, sd=None, emt=None) == 0
    torch.cuda.synchronize()
    for t in (out, so, cr, ci):
        assert (_np(t) == -7).all()
    assert int(cc.item()) == 0
    assert q(so_=P["so"], comp=full, flags=a.LIGHT_USE_HINTS | a.PARAM_AREA_LIGHTS) == 0
    torch.cuda.synchronize()
    assert (_np(out) == 0).all() and int(cc.item()) == 0 and (_np(cr) == -7).all()  # miss records: zeros, nothing appended
    assert (_np(so).view(np.uint32) == LCG_C).all()  # and still their one draw
    assert e(so_=P["so"]) == 0
    torch.cuda.synchronize()
    assert (_np(out).view(np.float32)[:, 7] == F(1e38)).all()
    ctx.close()
    # the first call that needs the emitter table must not be inside a capture
    ctx = pkg.Context(0)
    ctx.set_scene(scene.desc)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        pad = torch.zeros(1, device="cuda")
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        g.capture_begin()
        pad.add_(1)
        d = a.LightDesc()
        d.mode, d.num, d.flags, d.minT, d.seeds, d.emits = a.LIGHT_EMIT, n, a.PARAM_AREA_LIGHTS, 1e-4, P["sd"], P["o"]
        rc = lib.bdpt_light_query(ctx._h, C.byref(d), C.c_void_p(side.cuda_stream))
        g.capture_end()
    assert rc == -2
    torch.cuda.synchronize()
    del g
    ctx.close()
    scene.close()


def test_captured_query_and_trace(pkg):
    """sample_lights with hints and compaction, then trace_rays(any) over the compacted list with its device count, captured
    into one graph on one stream (the table prepared before the capture): two replays equal the eager run per item (the
    order inside the list is unspecified), and capturing allocates nothing."""
    import torch
    scene, pipe = _atrium_pipe(pkg, seed=4)
    ctx = pipe.ctx
    ctx.prepare(pkg.abi.PREPARE_AREA_LIGHTS)
    n = W * H
    surf = _eye_surfaces(pipe)
    seeds = _gpu((np.arange(n, dtype=np.uint32) * np.uint32(747796405)).view(np.int32))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()

    def buffers():
        return dict(rec=torch.zeros((n, 12), device="cuda"), so=torch.zeros(n, dtype=torch.int32, device="cuda"),
                    cr=torch.zeros((n, 8), device="cuda"), ci=torch.zeros(n, dtype=torch.int32, device="cuda"),
                    cc=torch.zeros(1, dtype=torch.int32, device="cuda"), vis=torch.zeros(n, dtype=torch.uint8, device="cuda"))

    def loop(b, st):
        b["cc"].zero_()
        ctx.sample_lights(surf, seeds, mat_index=0, min_t=pipe.min_t, area_lights=True, use_hints=True, out=b["rec"], seeds_out=b["so"],
                          compact=(b["cr"], b["ci"], b["cc"]), stream=st)
        ctx.trace_rays(b["cr"], "any", out=b["vis"], count=b["cc"], stream=st)

    def per_item(b):
        k = int(b["cc"].item())
        v = np.full(n, 2, np.uint8)
        v[_np(b["ci"])[:k]] = _np(b["vis"])[:k]
        return k, v

    with torch.cuda.stream(side):
        st = C.c_void_p(side.cuda_stream)
        eager, cap = buffers(), buffers()
        loop(eager, st)
        side.synchronize()
        pad = torch.zeros(1, device="cuda")
        trivial = torch.cuda.CUDAGraph()
        trivial.capture_begin()
        pad.add_(1)
        trivial.capture_end()
        alloc = torch.cuda.memory_allocated()
        graph = torch.cuda.CUDAGraph()
        graph.capture_begin()
        loop(cap, st)
        graph.capture_end()
        assert torch.cuda.memory_allocated() == alloc  # the loop allocates nothing
    torch.cuda.synchronize()
    assert not cap["rec"].any()  # captured, not run
    ke, ve = per_item(eager)
    assert 0 < ke < n and 0 < (ve == 0).sum() and 0 < (ve == 1).sum()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for k in ("rec", "so"):
            assert torch.equal(cap[k].view(torch.uint8), eager[k].view(torch.uint8)), k
        kc, vc = per_item(cap)
        assert kc == ke and np.array_equal(vc, ve)
    del graph, trivial
    pipe.close()
    scene.close()
