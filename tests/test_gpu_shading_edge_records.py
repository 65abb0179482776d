"""GPU tests of the shading queries on the edge-case records of tests/edge_records.py: bdpt_test_bsdf and bdpt_bsdf_query
against oracle_bsdf, bdpt_light_query against oracle_light_nee (NEE) and an fp32 numpy restatement (EMIT),
bdpt_connect_query against oracle_connect_vertices and oracle_connect_camera, bdpt_splat_add of the camera results on the
oracle's pixels.  Everything is compared bit for bit, except that a NaN must be a NaN in the same word (its sign and
payload are free, as in test_gpu_surface_queries._same); status words, pixels, light indices and output seeds must be
equal.  What the oracle itself is worth on these records is tests/test_shading_edge_records_cpu.py.

Every index a record's floats could reach (the light, the cube-map texel of a hint, the splat's pixel) is in range for
these families by the code (include/bdpt.h "record contract"), and the CPU tests bound the oracle's light and pixel
outputs before any of this runs."""
import numpy as np
import pytest

import edge_records as er
from test_gpu_connect_queries import _to_fixed
from test_gpu_light_queries import _cos_hemisphere

pytestmark = pytest.mark.gpu

F = er.F
MIN_T = 1e-4
NONZERO, HINT_OCCLUDED, PIXEL = 1, 2, 2
SIZES = (1, 63, 64, 65, 4099)


def _gpu(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _np(t):
    return t.cpu().numpy()


def _differs(a, b):
    """per row: some word differs (a NaN equals a NaN)"""
    if len(a) == 0:
        return np.zeros(0, bool)
    a, b = np.ascontiguousarray(a, F).reshape(len(a), -1), np.ascontiguousarray(b, F).reshape(len(b), -1)
    same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    return ~same.all(axis=1)


def _oracle_bsdf(pkg, ob, rec, code):
    out = np.zeros((len(rec), 16), F)
    ob.load_oracle(pkg.abi).oracle_bsdf(np.ascontiguousarray(rec).ctypes.data, len(rec), code, out.ctypes.data)
    return out


def _bsdf_mismatches(pkg, ob, ctx, b, code):
    """rows of a BsdfRecords batch where the hook or the query departs from oracle_bsdf"""
    import torch
    ref = _oracle_bsdf(pkg, ob, b.rec, code)
    bad = _differs(ctx.test_bsdf(b.rec, code), ref)
    st = _gpu(b.surf)
    samp = ctx.sample_bsdf(st, _gpu(b.seeds), mat_index=code & 1, from_lobe=bool(code & 2))
    vals = ctx.eval_bsdf(st, _gpu(b.dirs), mat_index=code & 1)
    torch.cuda.synchronize()
    samp, vals = _np(samp), _np(vals)
    hit = b.prim >= 0
    want_s = np.concatenate([ref[:, 3:7], ref[:, 0:3], ref[:, 7:8].astype(np.uint32).view(F)], axis=1)  # dir, pdf, weight, specular
    want_v = np.concatenate([ref[:, 8:11], np.zeros((b.n, 1), F)], axis=1)
    want_s[~hit], want_v[~hit] = 0, 0  # a miss: all-zero outputs
    return bad | _differs(samp, want_s) | _differs(vals, want_v)


@pytest.mark.parametrize("code", [0, 1, 2])
def test_bsdf_families_and_mixed_batch(pkg, ob, gpu_ctx, code):
    """bdpt_test_bsdf, bdpt_bsdf_query SAMPLE and EVAL against oracle_bsdf: matIndex 0, 1 and 2 (GGX with
    BDPT_PARAM_SPECULAR_FROM_LOBE), every family alone and the mixed batch."""
    scene = pkg.Scene.cornell()
    gpu_ctx.set_scene(scene.desc)
    failures = {}
    for name in er.bsdf_families():
        b = er.bsdf_records(name)
        bad = _bsdf_mismatches(pkg, ob, gpu_ctx, b, code)
        if bad.any():
            failures[name] = (int(bad.sum()), b.n)
    mixed = er.bsdf_mixed()
    bad = _bsdf_mismatches(pkg, ob, gpu_ctx, mixed, code)
    scene.close()
    assert not failures and not bad.any(), f"matIndex {code}: rows that differ from the oracle, per family alone (of) {failures}; in the " \
        f"mixed batch {mixed.tally(bad)}"


# ---- lights -----------------------------------------------------------------------------------------------------------
def _cases_by_scene(pkg, ctx):
    """the light cases, grouped by their light count so that the context changes scene three times: the Cornell box for
    one light, the two-triangle scene for three and four (bdpt_set_lights keeps a scene's count)"""
    cases = er.light_cases()
    for count in sorted({len(c.lights) for c in cases}):
        if count == 1:
            keep = pkg.Scene.cornell()
            assert keep.desc.numLights == 1
            ctx.set_scene(keep.desc)
        else:
            desc, keep = er.two_triangle_scene(pkg.abi, count)
            ctx.set_scene(desc)
        for c in cases:
            if len(c.lights) == count:
                yield c
        if hasattr(keep, "close"):
            keep.close()


def _word(rec):
    w = np.ascontiguousarray(rec).view(np.uint32)[:, 11]
    return w & 0xFFFF, w >> 16


@pytest.mark.parametrize("mat", [0, 1])
def test_light_nee_families(pkg, ob, gpu_ctx, mat):
    """BDPT_LIGHT_NEE on every light case against oracle_light_nee: ray, value, light, status and seedsOut; then with
    BDPT_LIGHT_USE_HINTS: every word but the HINT_OCCLUDED bit is unchanged, no record whose value lacks a positive component
    has that bit, and the compacted list holds exactly the items whose status is exactly NONZERO."""
    import torch
    failures = {}
    ctx = gpu_ctx
    for c in _cases_by_scene(pkg, ctx):
        lights = er.make_lights(pkg.abi, c.lights)
        ctx.set_lights(list(lights))
        ref, after = ob.light_nee(pkg.abi, lights, c.surf, c.seeds, mat, MIN_T)
        st, sd = _gpu(c.surf), _gpu(c.seeds)
        so = torch.zeros(c.n, dtype=torch.int32, device="cuda")
        plain = ctx.sample_lights(st, sd, mat_index=mat, min_t=MIN_T, seeds_out=so)
        cr = torch.full((c.n, 8), -7.0, dtype=torch.float32, device="cuda")
        ci = torch.full((c.n,), -7, dtype=torch.int32, device="cuda")
        cc = torch.zeros(1, dtype=torch.int32, device="cuda")
        hinted = ctx.sample_lights(st, sd, mat_index=mat, min_t=MIN_T, use_hints=True, compact=(cr, ci, cc))
        torch.cuda.synchronize()
        plain, hinted = _np(plain), _np(hinted)
        bad = _differs(plain, ref) | (_np(so).view(np.uint32) != after)
        light, status = _word(hinted)
        strip = hinted.copy()
        strip.view(np.uint32)[:, 11] &= ~np.uint32(HINT_OCCLUDED << 16)
        bad |= _differs(strip, plain)
        with np.errstate(invalid="ignore"):
            positive = (plain[:, 8:11] > 0).any(axis=1)
        bad |= ((status & HINT_OCCLUDED) != 0) & ~positive
        kc = int(cc.item())
        want = np.nonzero(status == NONZERO)[0]
        items = _np(ci)[:kc]
        listed = kc == len(want) and np.array_equal(np.sort(items), want) and not _differs(_np(cr)[:kc], hinted[items, 0:8]).any()
        if bad.any() or not listed:
            failures[c.name] = dict(c.tally(bad), compacted_list_ok=bool(listed))
    assert not failures, f"matIndex {mat}: rows that differ from oracle_light_nee, per light case and family {failures}"


def _emit_restatement(lib, lights, seeds):
    """sampleLight (BDPTUtils.hlsli:140-152) in fp32 numpy: (position, direction, colour, light, state after all draws)"""
    n, count = len(seeds), len(lights)
    s, r = er.lcg(seeds)
    index = np.minimum((r * F(count)).astype(np.int32), count - 1)
    pos = np.array([l["posW"] for l in lights], F)[index]
    inten = np.array([l["intensity"] for l in lights], F)[index]
    axis = np.array([l["dirW"] for l in lights], F)[index]
    todo = np.array([l["type"] != er.LIGHT_DIRECTIONAL for l in lights])[index]
    while todo.any():  # sampleUnitSphere: rounds of three draws until length(p) <= 1
        p = np.zeros((n, 3), F)
        s2 = s.copy()
        for k in range(3):
            s2, r = er.lcg(s2)
            p[:, k] = r * F(2.0) - F(1.0)
        s = np.where(todo, s2, s)
        axis[todo] = p[todo]
        todo = todo & (np.sqrt(er.dot3(p, p)) > F(1.0))
    s, r0 = er.lcg(s)
    s, r1 = er.lcg(s)
    with np.errstate(all="ignore"):
        d = _cos_hemisphere(lib, r0, r1, np.ascontiguousarray(axis))
    return pos, d, inten, index, s


def test_light_emit_selection_and_zero_dir(pkg, ob, gpu_ctx):
    """BDPT_LIGHT_EMIT with the selection-draw seeds (one, three and four lights) and on directional lights with unit, zero
    and non-unit dirW, against the fp32 restatement of sampleLight."""
    import torch
    lib = ob.load_oracle(pkg.abi)
    failures = {}
    ctx = gpu_ctx
    for c in _cases_by_scene(pkg, ctx):
        if not (c.name.startswith("selection") or c.name in ("directional", "one_point")):
            continue
        ctx.set_lights(list(er.make_lights(pkg.abi, c.lights)))
        so = torch.zeros(c.n, dtype=torch.int32, device="cuda")
        em = ctx.emit_lights(_gpu(c.seeds), min_t=MIN_T, seeds_out=so)
        torch.cuda.synchronize()
        em = _np(em)
        pos, d, inten, index, s = _emit_restatement(lib, c.lights, c.seeds)
        want = np.concatenate([pos, np.full((c.n, 1), MIN_T, F), d, np.full((c.n, 1), 1e38, F), inten, index.astype(np.uint32).view(F)[:, None]], axis=1)
        bad = _differs(em, want) | (_np(so).view(np.uint32) != s)
        assert set(index) == set(range(len(c.lights)))
        if bad.any():
            failures[c.name] = c.tally(bad)
    assert not failures, failures


# ---- connections --------------------------------------------------------------------------------------------------------
def _vertex_mismatches(pkg, ob, ctx, v, mat, with_prev):
    import torch
    ep, lp = (v.eye_prev, v.light_prev) if with_prev else (None, None)
    ref = ob.connect_vertices(pkg.abi, v.eye, v.light, mat, MIN_T, ep, lp, v.eye_spec, v.light_spec)
    got = ctx.connect_vertices(_gpu(v.eye), _gpu(v.light), mat_index=mat, min_t=MIN_T, eye_prev=None if ep is None else _gpu(ep),
                               light_prev=None if lp is None else _gpu(lp), eye_specular=_gpu(v.eye_spec), light_specular=_gpu(v.light_spec))
    torch.cuda.synchronize()
    return _differs(_np(got), ref)


@pytest.mark.parametrize("with_prev", [False, True])
@pytest.mark.parametrize("mat", [0, 1])
def test_connect_vertices_families_and_mixed_batch(pkg, ob, gpu_ctx, mat, with_prev):
    """BDPT_CONNECT_VERTICES against oracle_connect_vertices: ray, value and status, with NULL and with explicit
    predecessors, every family alone and the mixed batch."""
    scene = pkg.Scene.cornell()
    gpu_ctx.set_scene(scene.desc)
    failures = {}
    for name in er.vertex_families():
        v = er.vertex_records(name)
        bad = _vertex_mismatches(pkg, ob, gpu_ctx, v, mat, with_prev)
        if bad.any():
            failures[name] = (int(bad.sum()), v.n)
    mixed = er.vertex_mixed()
    bad = _vertex_mismatches(pkg, ob, gpu_ctx, mixed, mat, with_prev)
    scene.close()
    assert not failures and not bad.any(), f"matIndex {mat}, predecessors {with_prev}: rows that differ from the oracle, per family alone " \
        f"(of) {failures}; in the mixed batch {mixed.tally(bad)}"


def _clamp_vec(v, hi):
    y = np.where(v > 0, v, F(0))
    return np.where(y < hi, y, hi).astype(F)


@pytest.mark.parametrize("mat", [0, 1])
@pytest.mark.parametrize("frame", range(len(er.FRAMES)))
def test_connect_camera_mixed_batch_and_its_splats(pkg, ob, gpu_ctx, frame, mat):
    """BDPT_CONNECT_CAMERA on 17 x 9 and 16 x 8 frames, without and with jitter, against oracle_connect_camera: ray, f, G,
    pixel and status of the mixed batch (every family, labelled).  Then bdpt_splat_add of the clamped terms
    clampVec((prevColor * f) * G / 2, 0.9) at the kernel's pixels gives the words an integer restatement of toFixed gives at
    the oracle's pixels."""
    import torch
    W, H, jit = er.FRAMES[frame]
    scene = pkg.Scene.cornell()
    gpu_ctx.set_scene(scene.desc)
    cam = er.origin_camera(pkg.abi)
    gpu_ctx.set_camera(cam)
    m = er.camera_mixed(er.camera_of(cam), W, H, jit)
    ref = ob.connect_camera(pkg.abi, cam, W, H, jit, m.light, mat, MIN_T, m.light_spec)
    got = gpu_ctx.connect_camera(_gpu(m.light), W, H, pixel_jitter=jit, mat_index=mat, min_t=MIN_T, light_specular=_gpu(m.light_spec))
    torch.cuda.synchronize()
    bad = _differs(_np(got), ref)
    assert not bad.any(), f"frame {er.FRAMES[frame]} matIndex {mat}: rows that differ from the oracle per family {m.tally(bad)}"
    # the splats: the kernel's pixel column goes in as it is
    rng = np.random.default_rng(9)
    prev = rng.uniform(0.1, 1.0, (m.n, 3)).astype(F)
    with np.errstate(all="ignore"):
        term = _clamp_vec(((prev * ref[:, 8:11]) * ref[:, 11:12]) / F(2.0), F(0.9))
    values = np.concatenate([term, np.zeros((m.n, 1), F)], axis=1)
    splat = torch.zeros((W * H, 4), dtype=torch.int64, device="cuda")
    gpu_ctx.splat_add(splat, got.view(torch.int32)[:, 12].contiguous(), _gpu(values))
    torch.cuda.synchronize()
    want = [[0, 0, 0, 0] for _ in range(W * H)]
    pix = ref.view(np.uint32)[:, 12]
    assert ((pix < W * H) | (pix == 0xFFFFFFFF)).all()
    for k in np.nonzero(pix != 0xFFFFFFFF)[0]:
        for ch in range(3):
            if values[k, ch] > 0:
                want[pix[k]][ch] += _to_fixed(values[k, ch])
        want[pix[k]][3] += 1
    assert np.array_equal(_np(splat).view(np.uint64), np.array(want, dtype=np.uint64))
    assert sum(w[3] for w in want) > 0
    scene.close()


# ---- batch sizes: a wave, its neighbours, many waves; a device count below num ----------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_batch_sizes_and_device_counts(pkg, ob, gpu_ctx, size):
    """The first `size` records of each mixed batch with numDevice = size - size // 3 (size 1: 0): the counted items equal the
    oracle's, the tail of every output stays as it was."""
    import torch
    scene = pkg.Scene.cornell()
    gpu_ctx.set_scene(scene.desc)
    cam = er.origin_camera(pkg.abi)
    gpu_ctx.set_camera(cam)
    m = size - max(1, size // 3)
    cnt = torch.tensor([m], dtype=torch.int32, device="cuda")

    def out(cols):
        return torch.full((size, cols), -7, dtype=torch.int32, device="cuda")

    def check(got, ref, what):
        g = _np(got).view(np.uint32)
        assert not _differs(g[:m].view(F), ref[:m]).any(), (what, size)
        assert (g[m:].view(np.int32) == -7).all(), (what, size)

    b = er.bsdf_mixed()
    oracle = _oracle_bsdf(pkg, ob, b.rec[:size], 2)
    hit = (b.prim[:size] >= 0)[:, None]
    st = _gpu(b.surf[:size])
    o = out(8)
    gpu_ctx.sample_bsdf(st, _gpu(b.seeds[:size]), mat_index=0, from_lobe=True, out=o, count=cnt)
    check(o, np.where(hit, np.concatenate([oracle[:, 3:7], oracle[:, 0:3], oracle[:, 7:8].astype(np.uint32).view(F)], axis=1), F(0)), "sample")
    o = torch.full((size, 4), -7.0, dtype=torch.float32, device="cuda")
    gpu_ctx.eval_bsdf(st, _gpu(b.dirs[:size]), mat_index=0, out=o, count=cnt)
    torch.cuda.synchronize()
    g = _np(o)
    assert not _differs(g[:m], np.where(hit, np.concatenate([oracle[:, 8:11], np.zeros((size, 1), F)], axis=1), F(0))[:m]).any(), ("eval", size)
    assert (g[m:] == -7.0).all(), ("eval", size)

    v = er.vertex_mixed()
    ref = ob.connect_vertices(pkg.abi, v.eye[:size], v.light[:size], 0, MIN_T, v.eye_prev[:size], v.light_prev[:size], v.eye_spec[:size],
                              v.light_spec[:size])
    o = out(12)
    gpu_ctx.connect_vertices(_gpu(v.eye[:size]), _gpu(v.light[:size]), mat_index=0, min_t=MIN_T, eye_prev=_gpu(v.eye_prev[:size]),
                             light_prev=_gpu(v.light_prev[:size]), eye_specular=_gpu(v.eye_spec[:size]), light_specular=_gpu(v.light_spec[:size]),
                             out=o, count=cnt)
    torch.cuda.synchronize()
    check(o, ref, "vertices")

    W, H, jit = er.FRAMES[2]
    c = er.camera_mixed(er.camera_of(cam), W, H, jit)
    ref = ob.connect_camera(pkg.abi, cam, W, H, jit, c.light[:size], 0, MIN_T, c.light_spec[:size])
    o = out(16)
    gpu_ctx.connect_camera(_gpu(c.light[:size]), W, H, pixel_jitter=jit, mat_index=0, min_t=MIN_T, light_specular=_gpu(c.light_spec[:size]),
                           out=o, count=cnt)
    torch.cuda.synchronize()
    check(o, ref, "camera")

    lc = er.light_cases()[0]  # one light: the Cornell box has one
    idx = np.arange(size) % lc.n
    lights = er.make_lights(pkg.abi, lc.lights)
    gpu_ctx.set_lights(list(lights))
    ref, after = ob.light_nee(pkg.abi, lights, lc.surf[idx], lc.seeds[idx], 0, MIN_T)
    o = out(12)
    so = torch.full((size,), -7, dtype=torch.int32, device="cuda")
    gpu_ctx.sample_lights(_gpu(lc.surf[idx]), _gpu(lc.seeds[idx]), mat_index=0, min_t=MIN_T, out=o, seeds_out=so, count=cnt)
    torch.cuda.synchronize()
    check(o, ref, "lights")
    s = _np(so)
    assert np.array_equal(s[:m].view(np.uint32), after[:m]) and (s[m:] == -7).all(), ("seedsOut", size)
    scene.close()
