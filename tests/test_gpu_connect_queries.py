"""GPU tests of the connection queries (csrc/connect_query.hip): bdpt_connect_query in its VERTICES and CAMERA modes and
bdpt_splat_add.  Every comparison is bit for bit, on the float words viewed as integers, and the yardstick is bdpt_execute:
both random walks are composed from the queries (emit_lights / sample_bsdf / trace_rays / shade_hits), and the composed
connection and light-tracing strategies must reproduce the pass's connection-only frame (NO_NEE | NO_SPLAT) and its
splat-only frame (NO_NEE | NO_CONNECT | DEFER_RESOLVE: the fixed-point splat buffer and the resolved image)."""
import ctypes as C

import numpy as np
import pytest

from area_scenes import DEFER_RESOLVE, LCG_INV, NO_CONNECT, NO_NEE, NO_SPLAT, AreaScene, bits

pytestmark = pytest.mark.gpu

F = np.float32
LCG_C = 1013904223
NONZERO, PIXEL = 1, 2


def _gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _lcg_back(s1):
    """the state one nextRand before s1"""
    x = (s1.astype(np.uint64) + ((1 << 32) - LCG_C)) % (1 << 32)
    return ((x * LCG_INV) % (1 << 32)).astype(np.uint32)


def _pixel_states(ctx, n, frame_count):
    """initRand(pix, frameCount) of pixels 0 .. n-1: bdpt_test_rng gives the state after the first draw; one LCG step back"""
    st, _ = ctx.test_rng(np.arange(n, dtype=np.uint32), np.full(n, frame_count & 0xFFFFFFFF, np.uint32), 1)
    return _lcg_back(st[:, 0])


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _normalize(v):
    inv = F(1.0) / np.sqrt(_dot(v, v))
    return v * inv[:, None]


def _saturate(x):
    y = np.where(x > 0, x, F(0))
    return np.where(y < 1, y, F(1)).astype(F)


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


def _prim(rec):
    return rec.view(np.int32)[:, 23]


def _walk(pipe, first, first_alive, first_color, first_dir, first_spec, seeds_t, D, eye):
    """The walk of the pass from vertex `k0` (eye: vertex 1 from the G-buffer; light: vertex 0 from emit_lights) through the
    queries: trace_rays closest with tmin = minT, shade_hits without the normal map (seen from the ray's origin), sample_bsdf
    with the path's seed by value, the colour the running product.  A miss follows shootRay / RayMiss: the next vertex is a
    ghost, a copy of its predecessor with colour 0 (the eye walk's first ghost keeps initPayload's values: only the
    position), and the walk stops; later vertices do not exist (all-zero records with prim -1).
    Returns per vertex index: record (prim >= 0 where it is stored, ghosts included), colour, specular byte, `real` and
    `ghost` masks."""
    import torch
    k0 = 1 if eye else 0
    n = first.shape[0]
    vertex, color, spec = {k0: first}, {k0: first_color.copy()}, {k0: first_spec.copy()}
    real, ghost = {k0: first_alive.copy()}, {k0: np.zeros(n, bool)}
    payload, pspec = first.copy(), first_spec.copy()
    if eye:  # initPayload: posW = the origin, the rest 0
        payload = np.zeros((n, 24), F)
        payload[:, 0:3] = first[:, 0:3]
        pspec = np.zeros(n, np.uint8)
    pcolor, L, alive = first_color.copy(), first_dir.copy(), first_alive.copy()
    for k in range(k0, D):
        rays = np.zeros((n, 8), F)
        rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = payload[:, 0:3], F(pipe.min_t), L, F(1e38)
        rays[~alive] = 0
        rt = _gpu(rays)
        hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        pipe.trace_rays(rt, "closest", out=hits)
        new = pipe.shade_hits(rt, hits, normal_map=False)
        smp = _np(pipe.sample_bsdf(new, seeds_t))
        new = _np(new)
        hit = alive & (_prim(new) >= 0)
        payload = np.where(hit[:, None], new, payload)
        pspec = np.where(hit, smp.view(np.uint32)[:, 7].astype(np.uint8), pspec)
        with np.errstate(all="ignore"):
            pcolor = np.where(hit[:, None], pcolor * smp[:, 4:7], F(0)).astype(F)
        L = np.where(hit[:, None], smp[:, 0:3], L)
        v = payload.copy()
        _prim(v)[:] = np.where(alive, np.maximum(_prim(v), 0), -1)  # a ghost is stored: computed; none: -1
        v[~alive, 0:23] = 0
        vertex[k + 1], color[k + 1], spec[k + 1] = v, pcolor.copy(), np.where(alive, pspec, 0).astype(np.uint8)
        real[k + 1], ghost[k + 1] = hit, alive & ~hit
        alive = hit
    return vertex, color, spec, real, ghost


_CORNELL = {}


def _scene(pkg, which):
    if which == "cornell":
        if "base" not in _CORNELL:
            _CORNELL["base"] = pkg.Scene.cornell()
        return AreaScene(pkg, _CORNELL["base"], point_light=True, relit=True), 72, 56
    return pkg.Scene.atrium(1, 30000), 96, 54


def _splat_words(pipe):
    import torch
    ptr, n64 = pipe.ctx.splat_buffer()
    spl = torch.empty(n64, dtype=torch.int64, device=pipe.dev)
    torch.cuda.synchronize()
    assert C.CDLL("libamdhip64.so").hipMemcpy(C.c_void_p(spl.data_ptr()), C.c_void_p(ptr), C.c_size_t(n64 * 8), 3) == 0
    return ptr, spl.cpu().numpy().view(np.uint64).reshape(-1, 4)


def _pass_frame(pipe, extra):
    """frame 0 of the pipeline with `extra` flags: (params, out (n, 4), counters)"""
    import torch
    pipe.gbuffer_frame = pipe.bdpt_frame = 0
    _, p = pipe.render_frame(extra_flags=extra)
    torch.cuda.synchronize()
    return p, _np(pipe.output).reshape(-1, 4).copy(), pipe.ctx.counters().as_dict()


_SETUP = {}


def _setup(pkg, which, mat, D, lobe=False):
    """One pipeline per configuration, kept for the module: the pass's two frames and both walks composed from the queries."""
    import torch
    key = (which, mat, D, lobe)
    if key in _SETUP:
        return _SETUP[key]
    scene, W, H = _scene(pkg, which)
    pipe = pkg.FramePipeline(scene, W, H, max_depth=D, mat_index=mat, flags=pkg.abi.PARAM_SPECULAR_FROM_LOBE if lobe else 0)
    n = W * H
    s = dict(pipe=pipe, n=n, D=D, W=W, H=H)
    p, s["conn_ref"], s["conn_cnt"] = _pass_frame(pipe, NO_NEE | NO_SPLAT)
    p, s["splat_out"], s["splat_cnt"] = _pass_frame(pipe, NO_NEE | NO_CONNECT | DEFER_RESOLVE)
    ptr, s["splat_ref"] = _splat_words(pipe)
    pipe.ctx.resolve(C.c_void_p(ptr), 0, C.c_void_p(pipe.output.data_ptr()), pipe._stream_ptr())
    torch.cuda.synchronize()
    s["resolved_ref"] = _np(pipe.output).reshape(n, 4).copy()
    s["p"], s["hi"] = p, F(p.clampUpper)
    surf, valid, dif, emis = _surfaces_from_gbuffer(pipe)
    s["valid"], s["start"] = valid, _start_image(valid, dif, emis)
    s["cam"] = np.array(pipe.cam.posW[:], F)
    seed0 = _gpu(_pixel_states(pipe.ctx, n, p.frameCount).view(np.int32))
    seedL = torch.empty(n, dtype=torch.int32, device="cuda")
    em = _np(pipe.emit_lights(seed0, seeds_out=seedL))
    # eye walk: vertex 1 from the G-buffer, its sample from the pixel's initRand state
    s1 = _np(pipe.sample_bsdf(_gpu(surf), seed0))
    s["eye"] = _walk(pipe, surf, valid, s1[:, 4:7], s1[:, 0:3], s1.view(np.uint32)[:, 7].astype(np.uint8), seed0, D, eye=True)
    s["eye"][1][0] = np.ones((n, 3), F)  # cameraPath[0].color
    # light walk: vertex 0 is the light (every field but position and colour zero), only for valid pixels
    v0 = np.zeros((n, 24), F)
    v0[:, 0:3] = em[:, 0:3]
    v0[~valid] = 0
    _prim(v0)[:] = np.where(valid, 0, -1)
    c0 = np.where(valid[:, None], em[:, 8:11], F(0)).astype(F)
    s["light"] = _walk(pipe, v0, valid, c0, em[:, 4:7], np.zeros(n, np.uint8), seedL, D, eye=False)
    _SETUP[key] = s
    return s


CONFIGS = [("cornell", 0, False), ("cornell", 1, False), ("atrium", 0, False), ("atrium", 1, False), ("cornell", 0, True)]


def _torch_clamped(torch, v, k, hi):
    """clampVec(v / k, hi) with torch ops: a tensor divisor (a Python scalar would multiply by a reciprocal), NaN -> 0"""
    q = v / torch.full_like(v, float(k))
    zero = torch.zeros_like(q)
    y = torch.where(q > 0, q, zero)
    return torch.where(y < hi, y, torch.full_like(y, float(hi)))


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("which,mat,lobe", CONFIGS)
def test_composed_splat_frame_equals_the_pass(pkg, which, mat, lobe, D):
    """For every real light vertex t + 1: CAMERA mode with compaction -> trace_rays(any) over the compact list ->
    clampVec(((color[t] * f) * G) / (t + 2)) with torch ops -> splat_add with the item list.  Every uint64 of the composed
    buffer equals bdpt_splat_buffer of the pass's NO_NEE | NO_CONNECT | DEFER_RESOLVE frame, the resolved images agree in
    every pixel, the PIXEL items are the pass's raysSplat + hintedSplat and the landed entries its splatsLanded."""
    import torch
    s = _setup(pkg, which, mat, D, lobe)
    pipe, n, p = s["pipe"], s["n"], s["p"]
    vertex, color, spec, real, _ = s["light"]
    own = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    pixel_items = landed = 0
    for t in range(D):
        rec = vertex[t + 1].copy()
        rec[~real[t + 1]] = 0
        _prim(rec)[~real[t + 1]] = -1
        cr = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
        ci = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        cc = torch.zeros(1, dtype=torch.int32, device="cuda")
        cv = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        cam = pipe.connect_camera(_gpu(rec), pixel_jitter=(p.pixelJitter[0], p.pixelJitter[1]), light_specular=_gpu(spec[t + 1]),
                                  compact=(cr, ci, cc))
        pipe.trace_rays(cr, "any", out=cv, count=cc)
        term = _torch_clamped(torch, (_gpu(color[t]) * cam[:, 8:11]) * cam[:, 11:12], t + 2, float(s["hi"]))
        values = torch.cat([term, torch.zeros((n, 1), device="cuda")], dim=1).contiguous()
        pixels = cam.view(torch.int32)[:, 12].contiguous()
        pipe.splat_add(own, pixels, values, visible=cv, items=ci, count=cc)
        torch.cuda.synchronize()
        c, k = _np(cam), int(cc.item())
        status, pix = c.view(np.uint32)[:, 13], c.view(np.uint32)[:, 12]
        has = (status & PIXEL) != 0
        assert np.array_equal(np.sort(_np(ci)[:k]), np.nonzero(has)[0]) and (_np(ci)[k:] == -1).all()
        assert not has[~real[t + 1]].any() and (pix[has] < n).all() and (pix[~has] == 0xFFFFFFFF).all()
        assert (c[~has, 8:12].view(np.uint32) == 0).all()
        pixel_items += k
        landed += int((_np(cv)[:k] != 0).sum())
    got = _np(own).view(np.uint64)
    diff = (got != s["splat_ref"]).any(axis=1)
    assert not diff.any(), f"{int(diff.sum())} of {n} splat pixels differ, first {int(np.argmax(diff))}"
    cnt = s["splat_cnt"]
    print(f"{which} mat {mat} D {D}: PIXEL items {pixel_items}, raysSplat {cnt['raysSplat']}, hintedSplat {cnt['hintedSplat']}, "
          f"landed {landed}, splatsLanded {cnt['splatsLanded']}")
    assert pixel_items == cnt["raysSplat"] + cnt["hintedSplat"]
    assert landed == cnt["splatsLanded"] == int(got[:, 3].sum()) and cnt["splatsLanded"] > 0
    assert np.array_equal(bits(s["splat_out"]), bits(s["start"]))  # the deferred frame is the start image
    img = _gpu(s["start"])
    pipe.ctx.resolve(C.c_void_p(own.data_ptr()), 0, C.c_void_p(img.data_ptr()), pipe._stream_ptr())
    torch.cuda.synchronize()
    diff = (bits(img) != bits(s["resolved_ref"])).any(axis=1)
    assert not diff.any(), f"{int(diff.sum())} of {n} resolved pixels differ, first {int(np.argmax(diff))}"
    # the context's own buffer takes the same call: the last vertex's entries once more, on top of the pass's sums
    last = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    pipe.splat_add(last, pixels, values, visible=cv, items=ci, count=cc)
    pipe.splat_add(pipe.ctx.splat_buffer(), pixels, values, visible=cv, items=ci, count=cc)
    torch.cuda.synchronize()
    assert last.any() and np.array_equal(_splat_words(pipe)[1], s["splat_ref"] + _np(last).view(np.uint64))


def _pairs(D):
    """the pass's slot order: total length, then camera length; (c, l = 0) pairs are traced but never evaluated"""
    return [(t, c, t - c) for t in range(2, D + 1) for c in range(1, min(t, D - 1) + 1)]


def _pair_inputs(s, c, l):
    """eye vertex c and light vertex l of every pixel with their predecessors' positions and specular bytes"""
    n = s["n"]
    ev, ecol, espec, _, _ = s["eye"]
    lv, lcol, lspec, _, _ = s["light"]
    eprev = np.zeros((n, 4), F)
    eprev[:, 0:3] = s["cam"][None] if c == 1 else ev[c - 1][:, 0:3]
    lprev = np.zeros((n, 4), F)
    light = lv[l].copy()
    if l == 0:
        _prim(light)[:] = -1  # never evaluated (BDPTMain.rt.hlsl:217): only its ray
    else:
        lprev[:, 0:3] = lv[l - 1][:, 0:3]
    return ev[c], light, eprev, lprev, espec[c], lspec[l], lcol[c - 1], ecol[c - 1]


def _compose_connections(s):
    """every pair through VERTICES mode and trace_rays(any): per pair (term (n, 3), visible (n,), sample (n, 12))"""
    import torch
    if "pairs" in s:
        return s["pairs"]
    pipe, n, valid = s["pipe"], s["n"], s["valid"]
    res = []
    for t, c, l in _pairs(s["D"]):
        eye, light, eprev, lprev, es, ls, aL, aE = _pair_inputs(s, c, l)
        smp = pipe.connect_vertices(_gpu(eye), _gpu(light), eye_prev=_gpu(eprev), light_prev=_gpu(lprev), eye_specular=_gpu(es),
                                    light_specular=_gpu(ls))
        vis = pipe.trace_rays(smp[:, 0:8].contiguous(), "any")
        torch.cuda.synchronize()
        smp = _np(smp)
        with np.errstate(all="ignore"):
            term = _clamp_vec(((aL * smp[:, 8:11]) * aE) / F(t), s["hi"])
        term[~valid] = 0
        res.append((term, (_np(vis) != 0) & valid, smp))
    s["pairs"] = res
    return res


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("which,mat,lobe", CONFIGS)
def test_composed_connection_frame_equals_the_pass(pkg, which, mat, lobe, D):
    """Every pair in the pass's slot order through VERTICES mode, the rays of ALL pairs traced, then the gather rule in
    numpy: a visible pair with a non-zero term does a saturating add of rgb and w; a pixel with none of those is saturated
    once (+0, w + 1) when any zero-valued pair is visible.  Every pixel equals the pass's NO_NEE | NO_SPLAT frame, the items
    with a non-zero term are its raysConnect - raysConnectLazy, and at depth 3 every kind of pixel occurs."""
    s = _setup(pkg, which, mat, D, lobe)
    n, valid = s["n"], s["valid"]
    pairs = _compose_connections(s)
    out = s["start"].copy()
    sat = np.zeros(n, bool)
    any_vis = np.zeros(n, bool)
    nonzero = 0
    for term, vis, _ in pairs:
        nz = (term != 0).any(axis=1)
        nonzero += int(nz.sum())
        add = vis & nz
        out[add, 0:3] = _saturate(out[add, 0:3] + term[add])
        out[add, 3] = _saturate(out[add, 3] + F(1))
        sat |= add
        any_vis |= vis
    only = any_vis & ~sat
    out[only, 0:3] = _saturate(out[only, 0:3] + F(0))
    out[only, 3] = _saturate(out[only, 3] + F(1))
    diff = (bits(out) != bits(s["conn_ref"])).any(axis=1)
    assert not diff.any(), f"{int(diff.sum())} of {n} pixels differ, first {int(np.argmax(diff))}"
    cnt = s["conn_cnt"]
    changed = sat & (bits(out[:, 0:3]) != bits(s["start"][:, 0:3])).any(axis=1)
    untouched = valid & ~any_vis
    ghosts = sum(int(g.sum()) for g in list(s["eye"][4].values()) + list(s["light"][4].values()))
    print(f"{which} mat {mat} D {D}: non-zero terms {nonzero}, raysConnect {cnt['raysConnect']}, lazy {cnt['raysConnectLazy']}, "
          f"rgb changed {int(changed.sum())}, only saturated {int(only.sum())}, untouched valid {int(untouched.sum())}, "
          f"valid {int(valid.sum())} of {n}, ghost vertices {ghosts}")
    assert nonzero == cnt["raysConnect"] - cnt["raysConnectLazy"]
    if D == 3:
        assert changed.sum() > 0 and only.sum() > 0 and untouched.sum() > 0 and ghosts > 0


def _tiled(a, idx):
    return np.ascontiguousarray(a[idx])


@pytest.mark.parametrize("n", [65, 4097])
def test_per_item_results(pkg, n):
    """On Cornell items (valid pixels, repeated to n): the Lambertian value, G, pixel, direction and tmax against an fp32
    numpy restatement; NULL predecessors against explicit ones on real vertices (GGX); prim < 0 on either side; coincident
    points."""
    import torch
    # --- GGX: V in place of the predecessors, on real vertices (eye vertex 2 and light vertex 1, both from shade_hits)
    s = _setup(pkg, "cornell", 0, 3)
    pipe = s["pipe"]
    both = np.nonzero(s["eye"][3][2] & s["light"][3][1])[0]
    assert len(both) > 0
    idx = both[np.arange(n) % len(both)]
    eye, light, eprev, lprev, es, ls, _, _ = (_tiled(a, idx) for a in _pair_inputs(s, 2, 1))
    with_prev = pipe.connect_vertices(_gpu(eye), _gpu(light), eye_prev=_gpu(eprev), light_prev=_gpu(lprev))
    without = pipe.connect_vertices(_gpu(eye), _gpu(light))
    torch.cuda.synchronize()
    assert np.array_equal(bits(with_prev), bits(without))
    assert (_np(with_prev).view(np.uint32)[:, 11] == NONZERO).any()
    # --- Lambertian restatement
    s = _setup(pkg, "cornell", 1, 3)
    pipe = s["pipe"]
    sel = np.nonzero(s["valid"] & s["light"][3][1])[0]
    idx = sel[np.arange(n) % len(sel)]
    eye, light = _tiled(s["eye"][0][1], idx), _tiled(s["light"][0][1], idx)
    smp = _np(pipe.connect_vertices(_gpu(eye), _gpu(light)))
    ep, lp = eye[:, 0:3], light[:, 0:3]
    with np.errstate(all="ignore"):
        vec = lp - ep
        inv = F(1.0) / np.sqrt(_dot(vec, vec))
        dirg = vec * inv[:, None]
        gt = ((np.abs(_dot(eye[:, 4:7], dirg)) * np.abs(_dot(light[:, 4:7], dirg))) * inv) * inv
        value = (light[:, 12:15] * gt[:, None]) * eye[:, 12:15]
        tmax = np.sqrt(_dot(vec, vec))
        direc = vec / tmax[:, None]
    assert np.array_equal(bits(smp[:, 0:3]), bits(ep)) and (smp[:, 3] == F(pipe.min_t)).all()
    assert np.array_equal(bits(smp[:, 4:7]), bits(direc)) and np.array_equal(bits(smp[:, 7]), bits(tmax))
    assert np.array_equal(bits(smp[:, 8:11]), bits(value))
    assert np.array_equal(smp.view(np.uint32)[:, 11], (value != 0).any(axis=1).astype(np.uint32)) and (value != 0).any()
    # CAMERA mode
    p, W, H = s["p"], s["W"], s["H"]
    jit = (p.pixelJitter[0], p.pixelJitter[1])
    cam = _np(pipe.connect_camera(_gpu(light), pixel_jitter=jit))
    cpos = s["cam"]
    U, V, Wc = (np.array(getattr(pipe.cam, k)[:], F) for k in ("cameraU", "cameraV", "cameraW"))
    one = lambda v: np.broadcast_to(v[None], (n, 3))
    with np.errstate(all="ignore"):
        to = cpos[None] - lp
        d = _normalize(to)
        dist = np.sqrt(_dot(to, to))
        cn = _normalize(Wc[None])[0]
        facing = _dot(one(cn), d) < 0
        d1 = _dot(d, one(U)) / _dot(U[None], U[None])
        d2 = _dot(d, one(V)) / _dot(V[None], V[None])
        d3 = _dot(d, one(Wc)) / _dot(Wc[None], Wc[None])
        px, py = (d1 / d3) * F(0.5) + F(0.5), (-d2 / d3) * F(0.5) + F(0.5)
        fx, fy = np.rint(px * F(W) - F(jit[0])), np.rint(py * F(H) - F(jit[1]))
        inside = facing & (fx >= 0) & (fx < W) & (fy >= 0) & (fy < H)
        invd = F(1.0) / dist
        g = ((_saturate(np.abs(_dot(d, one(cn)))) * _saturate(np.abs(_dot(d, light[:, 4:7])))) * invd) * invd
    pix = np.where(inside, np.where(inside, fx, 0).astype(np.int64) + np.where(inside, fy, 0).astype(np.int64) * W, 0xFFFFFFFF).astype(np.uint32)
    assert 0 < inside.sum()
    assert np.array_equal(bits(cam[:, 0:3]), bits(lp)) and (cam[:, 3] == F(pipe.min_t)).all()
    assert np.array_equal(bits(cam[:, 4:7]), bits(d)) and np.array_equal(bits(cam[:, 7]), bits(dist))
    assert np.array_equal(cam.view(np.uint32)[:, 12], pix)
    assert np.array_equal(bits(cam[:, 11]), bits(np.where(inside, g, F(0))))
    assert np.array_equal(bits(cam[:, 8:11]), bits(np.where(inside[:, None], light[:, 12:15], F(0))))
    nz = inside & (light[:, 12:15] != 0).any(axis=1) & (g != 0)
    assert np.array_equal(cam.view(np.uint32)[:, 13], np.where(inside, PIXEL, 0) | np.where(nz, NONZERO, 0))
    assert (cam.view(np.uint32)[:, 14:16] == 0).all()
    # --- prim < 0 on either side: an all-zero value, the ray still formed; CAMERA: an all-zero sample without a pixel
    for side in (eye, light):
        keep = _prim(side).copy()
        _prim(side)[::3] = -1
        got = _np(pipe.connect_vertices(_gpu(eye), _gpu(light)))
        _prim(side)[:] = keep
        assert np.array_equal(bits(got[:, 0:8]), bits(smp[:, 0:8]))
        assert (got[::3, 8:12].view(np.uint32) == 0).all()
        rest = np.ones(n, bool)
        rest[::3] = False
        assert np.array_equal(bits(got[rest]), bits(smp[rest]))
    miss = light.copy()
    _prim(miss)[::2] = -1
    got = _np(pipe.connect_camera(_gpu(miss), pixel_jitter=jit)).view(np.uint32)
    assert (got[::2, 0:12] == 0).all() and (got[::2, 12] == 0xFFFFFFFF).all() and (got[::2, 13:16] == 0).all()
    assert np.array_equal(got[1::2], cam.view(np.uint32)[1::2])
    # --- coincident points: tmax 0, a NaN direction, and the any-hit query answers unoccluded
    same = pipe.connect_vertices(_gpu(eye), _gpu(eye))
    vis = pipe.trace_rays(same[:, 0:8].contiguous(), "any")
    torch.cuda.synchronize()
    same = _np(same)
    assert (same[:, 7] == 0).all() and np.isnan(same[:, 4:7]).all() and (_np(vis) == 1).all()


@pytest.mark.parametrize("mode", ["vertices", "camera"])
def test_compaction_and_counts(pkg, mode):
    """The lists hold exactly the NONZERO / PIXEL items, each once, with their rays; entries beyond the count are untouched;
    a device count below num leaves the tail of every output untouched; a compactCount left at num writes nothing."""
    import torch
    s = _setup(pkg, "cornell", 0, 3)
    pipe, n, p = s["pipe"], s["n"], s["p"]
    eye, light, eprev, lprev, es, ls, _, _ = (_gpu(a) for a in _pair_inputs(s, 1, 1))
    cols, bit = (12, NONZERO) if mode == "vertices" else (16, PIXEL)
    status_col = 11 if mode == "vertices" else 13

    def run(**kw):
        if mode == "vertices":
            return pipe.connect_vertices(eye, light, eye_prev=eprev, light_prev=lprev, **kw)
        return pipe.connect_camera(light, pixel_jitter=(p.pixelJitter[0], p.pixelJitter[1]), **kw)

    full = _np(run())
    want = (full.view(np.uint32)[:, status_col] & bit) != 0
    assert 0 < want.sum() < n
    for m in (None, 1000, 0, n + 5):
        cnt = None if m is None else torch.tensor([m], dtype=torch.int32, device="cuda")
        out = torch.full((n, cols), -7, dtype=torch.int32, device="cuda")
        cr = torch.full((n, 8), -7.0, dtype=torch.float32, device="cuda")
        ci = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        cc = torch.zeros(1, dtype=torch.int32, device="cuda")
        run(out=out, compact=(cr, ci, cc), count=cnt)
        torch.cuda.synchronize()
        k = n if m is None else min(m, n)
        g = _np(out).view(np.uint32)
        assert np.array_equal(g[:k], full.view(np.uint32)[:k]) and (g[k:].view(np.int32) == -7).all()
        kc = int(cc.item())
        items = _np(ci)[:kc]
        assert kc == int(want[:k].sum()) and np.array_equal(np.sort(items), np.nonzero(want[:k])[0])
        assert np.array_equal(bits(_np(cr)[:kc]), bits(full[items, 0:8]))
        assert (_np(ci)[kc:] == -7).all() and (_np(cr)[kc:] == -7.0).all()
    # the count word left at num: every position is at or beyond the capacity, nothing is written
    cr = torch.full((n, 8), -7.0, dtype=torch.float32, device="cuda")
    ci = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    cc = torch.full((1,), n, dtype=torch.int32, device="cuda")
    run(compact=(cr, ci, cc))
    torch.cuda.synchronize()
    assert int(cc.item()) == n + int(want.sum()) and (_np(ci) == -7).all() and (_np(cr) == -7.0).all()


def _to_fixed(c):
    """toFixed (device_math.hpp): (uint64)(c * 2^32) of a float32 > 0; exact in Python integers"""
    m = float(np.float32(c) * np.float32(4294967296.0))
    return int(m)


def test_splat_add_on_its_own(pkg):
    """70 000 entries onto 4096 pixels: repeated targets, visible zeros, out-of-range pixels, negative, NaN and zero
    channels, against a Python integer restatement of toFixed; two entry orders give the same words; with items and with a
    device count."""
    import torch
    rng = np.random.default_rng(7)
    n, npix = 70000, 4096
    ctx = pkg.Context(0)
    pixels = rng.integers(0, npix, n, dtype=np.uint32)
    pixels[::11] = rng.integers(npix, 2 ** 32, len(pixels[::11]), dtype=np.uint64).astype(np.uint32)
    pixels[5] = 0xFFFFFFFF
    pixels[6] = npix
    values = np.zeros((n, 4), F)
    values[:, 0:3] = rng.uniform(0.0, 0.9, (n, 3)).astype(F)
    values[:, 3] = 123.0  # never read
    values[::5, 0] = -values[::5, 0]
    values[::7, 1] = np.nan
    values[::13, 2] = 0.0
    values[3, 0:3] = (-0.0, 1e-12, 0.9)
    values[4, 0:3] = (-np.inf, np.nan, -1.0)
    visible = (rng.integers(0, 4, n) != 0).astype(np.uint8) * rng.integers(1, 255, n).astype(np.uint8)

    def expect(order, vis_by_entry, count):
        ref = [[0, 0, 0, 0] for _ in range(npix)]
        for j, k in enumerate(order[:count]):
            if vis_by_entry is not None and vis_by_entry[j] == 0:
                continue
            if pixels[k] >= npix:
                continue
            for ch in range(3):
                if values[k, ch] > 0:
                    ref[pixels[k]][ch] += _to_fixed(values[k, ch])
            ref[pixels[k]][3] += 1
        return np.array(ref, dtype=np.uint64)

    def run(px, vals, vis=None, items=None, count=None):
        splat = torch.zeros((npix, 4), dtype=torch.int64, device="cuda")
        ctx.splat_add(splat, _gpu(px.view(np.int32)), _gpu(vals), None if vis is None else _gpu(vis), None if items is None else _gpu(items),
                      None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        return _np(splat).view(np.uint64)

    ident = np.arange(n)
    ref = expect(ident, visible, n)
    assert ref[:, 3].max() > 1 and 0 < int(ref[:, 3].sum()) < n
    assert np.array_equal(run(pixels, values, visible), ref)
    perm = rng.permutation(n)
    assert np.array_equal(run(pixels[perm], values[perm], visible[perm]), ref)  # another order, the same words
    assert np.array_equal(run(pixels, values), expect(ident, None, n))           # no visible bytes
    items = rng.integers(0, n, 50000).astype(np.int32)                          # an index list (with repeats): visible by entry
    vis_e = visible[:50000]
    assert np.array_equal(run(pixels, values, vis_e, items), expect(items, vis_e, 50000))
    assert np.array_equal(run(pixels, values, vis_e, items, count=12345), expect(items, vis_e, 12345))
    assert np.array_equal(run(pixels, values, visible, count=n + 9), ref)
    assert not run(pixels, values, visible, count=0).any()
    ctx.close()


def test_frames_are_unchanged_by_the_queries(pkg):
    """frame, a burst of connection queries and splat_add into a caller's buffer, frame gives the image of two frames
    without them, bit for bit; counters and stage times the frame left are unchanged."""
    import torch
    W, H = 96, 64
    scene = pkg.Scene.atrium(3, 20000)
    imgs = []
    for with_queries in (True, False):
        pipe = pkg.FramePipeline(scene, W, H, max_depth=4, flags=pkg.abi.PARAM_COUNTERS)
        pipe.ctx.enable_stage_timing(True)
        pipe.render_frame()
        if with_queries:
            torch.cuda.synchronize()
            before = pipe.ctx.counters().as_dict()
            times = pipe.ctx.stage_times()
            n = W * H
            rays = pipe.camera_rays()
            hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
            pipe.trace_rays(rays, "closest_cull_back", out=hits)
            surf = pipe.shade_hits(rays, hits)
            other = surf.flip(0).contiguous()
            own = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
            for _ in range(2):
                cr = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
                ci = torch.zeros(n, dtype=torch.int32, device="cuda")
                cc = torch.zeros(1, dtype=torch.int32, device="cuda")
                pipe.connect_vertices(surf, other, compact=(cr, ci, cc))
                pipe.trace_rays(cr, "any", count=cc)
                cc.zero_()
                cam = pipe.connect_camera(other, compact=(cr, ci, cc))
                vis = pipe.trace_rays(cr, "any", count=cc)
                pipe.splat_add(own, cam.view(torch.int32)[:, 12].contiguous(), cam[:, 8:12].contiguous(), visible=vis, items=ci, count=cc)
            torch.cuda.synchronize()
            assert own.any()
            assert pipe.ctx.counters().as_dict() == before
            assert pipe.ctx.stage_times() == times
        pipe.render_frame()
        torch.cuda.synchronize()
        imgs.append(_np(pipe.output))
        pipe.close()
    assert np.array_equal(imgs[0].view(np.uint32), imgs[1].view(np.uint32))
    scene.close()


def test_captured_camera_query_trace_and_splat(pkg):
    """connect_camera with compaction -> trace_rays(any) over the list -> splat_add, captured into one graph on a side
    stream: two replays into a zeroed buffer equal the eager run, and capturing allocates nothing."""
    import torch
    s = _setup(pkg, "cornell", 0, 3)
    pipe, n, p = s["pipe"], s["n"], s["p"]
    ctx = pipe.ctx
    light = _gpu(s["light"][0][1])
    values = torch.full((n, 4), 0.25, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()

    def buffers():
        return dict(cam=torch.zeros((n, 16), device="cuda"), cr=torch.zeros((n, 8), device="cuda"),
                    ci=torch.zeros(n, dtype=torch.int32, device="cuda"), cc=torch.zeros(1, dtype=torch.int32, device="cuda"),
                    vis=torch.zeros(n, dtype=torch.uint8, device="cuda"), pix=torch.zeros(n, dtype=torch.int32, device="cuda"),
                    splat=torch.zeros((n, 4), dtype=torch.int64, device="cuda"))

    def loop(b, st):
        b["cc"].zero_()
        b["splat"].zero_()
        ctx.connect_camera(light, s["W"], s["H"], (p.pixelJitter[0], p.pixelJitter[1]), 0, pipe.min_t, out=b["cam"],
                           compact=(b["cr"], b["ci"], b["cc"]), stream=st)
        ctx.trace_rays(b["cr"], "any", out=b["vis"], count=b["cc"], stream=st)
        b["pix"].copy_(b["cam"].view(torch.int32)[:, 12])
        ctx.splat_add(b["splat"], b["pix"], values, visible=b["vis"], items=b["ci"], count=b["cc"], stream=st)

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
    assert not cap["cam"].any()  # captured, not run
    assert eager["splat"].any() and 0 < int(eager["cc"].item()) < n
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for k in ("cam", "splat", "cc"):
            assert torch.equal(cap[k].view(torch.uint8), eager[k].view(torch.uint8)), k
    del graph, trivial


def test_error_cases_through_the_c_abi(pkg):
    """every error case of both entry points returns its code and enqueues nothing: the outputs keep their sentinel"""
    import torch
    a = pkg.abi
    lib = pkg.load_library()
    scene = pkg.Scene.cornell()
    ctx = pkg.Context(0)
    n = 256
    surf = torch.zeros((n, 24), dtype=torch.float32, device="cuda")
    surf.view(torch.int32)[:, 23] = -1
    prev = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    out = torch.full((n, 16), -7, dtype=torch.int32, device="cuda")
    cr = torch.full((n, 8), -7, dtype=torch.int32, device="cuda")
    ci = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    cc = torch.zeros(1, dtype=torch.int32, device="cuda")
    splat = torch.full((n, 4), -7, dtype=torch.int64, device="cuda")
    pixels = torch.zeros(n, dtype=torch.int32, device="cuda")
    values = torch.ones((n, 4), dtype=torch.float32, device="cuda")
    P = dict(s=surf.data_ptr(), pv=prev.data_ptr(), o=out.data_ptr(), cr=cr.data_ptr(), ci=ci.data_ptr(), cc=cc.data_ptr(),
             sp=splat.data_ptr(), px=pixels.data_ptr(), va=values.data_ptr())

    def q(h=ctx._h, mode=a.CONNECT_VERTICES, num=n, cnt=None, mat=0, flags=0, reserved=0, eye=P["s"], light=P["s"], ep=None, lp=None,
          smp=P["o"], cam=None, w=0, hgt=0, comp=(None, None, None), desc=True):
        d = a.ConnectDesc()
        d.mode, d.num, d.numDevice, d.matIndex, d.flags, d.minT, d.reserved = mode, num, cnt, mat, flags, 1e-4, reserved
        d.eye, d.light, d.eyePrev, d.lightPrev, d.samples, d.cameraSamples, d.width, d.height = eye, light, ep, lp, smp, cam, w, hgt
        d.compactRays, d.compactItems, d.compactCount = comp
        return lib.bdpt_connect_query(h, C.byref(d) if desc else None, None)

    def c(**kw):
        kw.setdefault("eye", None)
        kw.setdefault("smp", None)
        kw.setdefault("cam", P["o"])
        kw.setdefault("w", 16)
        kw.setdefault("hgt", 16)
        return q(mode=a.CONNECT_CAMERA, **kw)

    def add(h=ctx._h, num=n, npix=n, cnt=None, px=P["px"], va=P["va"], vis=None, items=None, sp=P["sp"], desc=True):
        d = a.SplatDesc()
        d.num, d.numPixels, d.numDevice, d.pixels, d.values, d.visible, d.items, d.splat = num, npix, cnt, px, va, vis, items, sp
        return lib.bdpt_splat_add(h, C.byref(d) if desc else None, None)

    full = (P["cr"], P["ci"], P["cc"])
    assert q() == -2 and c() == -2  # BDPT_E_STATE: no scene
    ctx.set_scene(scene.desc)
    assert c() == -2                # BDPT_E_STATE: CAMERA without a camera
    assert q() == 0                 # VERTICES needs none
    torch.cuda.synchronize()
    flat = _np(out).reshape(-1)  # n records of 12 words at the start of the buffer
    assert (flat[:n * 12].reshape(n, 12)[:, 8:12] == 0).all() and (flat[n * 12:] == -7).all()  # miss records: a zero value
    out.fill_(-7)
    cam = a.Camera()
    for k, v in (("posW", (0, 0, 5)), ("cameraU", (1, 0, 0)), ("cameraV", (0, 1, 0)), ("cameraW", (0, 0, -1))):
        for i in range(3):
            getattr(cam, k)[i] = float(v[i])
    ctx.set_camera(cam)
    bad = [
        q(h=None), q(desc=False), q(mode=2), q(mat=2), q(flags=1), q(reserved=1), q(eye=None), q(eye=P["s"] + 4), q(light=None),
        q(light=P["s"] + 8), q(smp=None), q(smp=P["o"] + 4), q(ep=P["pv"] + 4), q(lp=P["pv"] + 8), q(cnt=P["ci"] + 2),
        q(comp=(P["cr"], None, None)), q(comp=(None, P["ci"], None)), q(comp=(None, None, P["cc"])), q(comp=(P["cr"], P["ci"], None)),
        q(comp=(P["cr"], None, P["cc"])), q(comp=(None, P["ci"], P["cc"])), q(comp=(P["cr"] + 8, P["ci"], P["cc"])),
        q(comp=(P["cr"], P["ci"] + 2, P["cc"])), q(comp=(P["cr"], P["ci"], P["cc"] + 1)),
        c(h=None), c(desc=False), c(mat=2), c(flags=2), c(reserved=7), c(light=None), c(light=P["s"] + 4), c(cam=None), c(cam=P["o"] + 8),
        c(w=0), c(hgt=0), c(w=65536, hgt=65536), c(cnt=P["ci"] + 1), c(comp=(P["cr"], None, None)), c(comp=(P["cr"] + 4, P["ci"], P["cc"])),
        q(num=0, mode=2), q(num=0, comp=(P["cr"], None, None)), c(num=0, w=0),  # (found before the empty call returns)
        add(h=None), add(desc=False), add(px=None), add(px=P["px"] + 2), add(va=None), add(va=P["va"] + 4), add(sp=None),
        add(sp=P["sp"] + 8), add(items=P["ci"] + 1), add(cnt=P["ci"] + 2),
    ]
    assert all(rc == -1 for rc in bad), bad
    assert q(num=0, eye=None, light=None, smp=None) == 0 and c(num=0, light=None, cam=None) == 0
    assert add(num=0, px=None, va=None, sp=None) == 0
    torch.cuda.synchronize()
    for t in (out, cr, ci, splat):
        assert (_np(t) == -7).all()
    assert int(cc.item()) == 0
    # and the good calls: miss records give zeros, append nothing, and an out-of-range pixel lands nothing
    assert c(comp=full) == 0 and add(npix=0) == 0
    torch.cuda.synchronize()
    g = _np(out).view(np.uint32)
    assert (g[:, 0:12] == 0).all() and (g[:, 12] == 0xFFFFFFFF).all() and (g[:, 13:] == 0).all()
    assert int(cc.item()) == 0 and (_np(cr) == -7).all() and (_np(splat) == -7).all()
    ctx.close()
    scene.close()
