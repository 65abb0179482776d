"""GPU tests of hit shading and the alpha tests on the edge-case records of tests/edge_surfaces.py.  Everything is compared
with the CPU oracle bit for bit (two NaNs count as equal whatever their payload): bdpt_shade_hits with oracle_shade_hits,
bdpt_test_alpha (alphaTestFails and both slots of alphaTestFails2) with oracle_alpha_test, exact rays straight down onto
the quads through bdpt_trace_rays, bdpt_test_trace and the persistent any-hit kernel with the oracle's linear scan,
bdpt_walk_query's vertices with oracle_shade_hits of the scan's hits, and frames of the finite part of the scene with
oracle_gbuffer / oracle_bdpt.  The oracle itself is held against float64 by tests/test_surface_edge_records_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import edge_surfaces as es
from test_gpu_surface_queries import _gpu, _same
from test_gpu_trace_rays import MODES, _check_all, _oracle, _to_bdpt

pytestmark = pytest.mark.gpu

NMAP = 1  # BDPT_SHADE_NORMAL_MAP
_cache = {}


def _world(pkg, ob, bare=False):
    """the scene, its oracle twin, the mixed batch and the oracle's records of it, made once and left unchanged"""
    if bare not in _cache:
        sc = es.EdgeScene(pkg.abi, bare=bare)
        lib = ob.load_oracle(pkg.abi)
        osc = lib.oracle_scene_create(C.byref(sc.desc))
        if bare:
            rng = np.random.default_rng(5)
            d = es._ordinary(rng, sc, 512)
            b = es.SurfaceRecords(d, np.zeros(512, np.int32), ["ordinary"])
        else:
            b = es.mixed(sc)
        ref = {fl: ob.shade_hits(pkg.abi, osc, b.rays, b.hits, fl) for fl in (0, NMAP)}
        for r in ref.values():
            r.setflags(write=False)
        _cache[bare] = (sc, lib, osc, b, ref)
    return _cache[bare]


def _differs(got, ref):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    return ~_same(np.ascontiguousarray(got, np.float32), ref).all(axis=1)


@pytest.mark.parametrize("bare", [False, True], ids=["edge_scene", "no_texcoords_no_bitangents"])
def test_shade_hits_every_word(pkg, ob, gpu_ctx, bare):
    """bdpt_shade_hits == oracle_shade_hits on the whole mix, without and with the normal map, from device and from host
    arrays, with and without numHitsDevice"""
    import torch
    sc, lib, osc, b, ref = _world(pkg, ob, bare)
    gpu_ctx.set_scene(sc.desc)
    rays, hits = _gpu(b.rays), _gpu(b.hits)
    for fl in (0, NMAP):
        s = gpu_ctx.shade_hits(rays, hits, normal_map=bool(fl))
        torch.cuda.synchronize()
        bad = _differs(s, ref[fl])
        assert not bad.any(), (fl, b.tally(bad))
        host = gpu_ctx.shade_hits(b.rays, b.hits, normal_map=bool(fl))
        assert isinstance(host, np.ndarray) and not _differs(host, ref[fl]).any(), fl
        # numHitsDevice: the first 1000 records are written, the rest of the buffer is left as it was
        cap = min(1000, b.n - 1)
        out = torch.full((b.n, 24), 7.0, dtype=torch.float32, device="cuda")
        gpu_ctx.shade_hits(rays, hits, normal_map=bool(fl), out=out, count=torch.tensor([cap], dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert not _differs(o[:cap], ref[fl][:cap]).any() and (o[cap:] == 7.0).all(), fl
    if not bare:  # the normal map is live, and only N differs with it
        n_cols = [4, 5, 6]
        d = ~_same(ref[0], ref[NMAP])
        assert d[:, n_cols].any() and not np.delete(d, n_cols, axis=1).any()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_shade_hits_batch_sizes(pkg, ob, gpu_ctx, n):
    """one record, and the wave width and one either side: n consecutive records of the mix, starting inside int_range"""
    import torch
    sc, lib, osc, b, ref = _world(pkg, ob)
    gpu_ctx.set_scene(sc.desc)
    start = int(np.flatnonzero(b.of("int_range"))[3])
    idx = (start + np.arange(n)) % b.n
    assert n < 63 or len(np.unique(b.family[idx])) > 4
    for fl in (0, NMAP):
        s = gpu_ctx.shade_hits(_gpu(b.rays[idx]), _gpu(b.hits[idx]), normal_map=bool(fl))
        torch.cuda.synchronize()
        assert not _differs(s, ref[fl][idx]).any(), (n, fl)


@pytest.mark.parametrize("variant", [0, 1, 2], ids=["alphaTestFails", "alphaTestFails2_slot0", "alphaTestFails2_slot1"])
def test_alpha_verdicts(pkg, ob, gpu_ctx, variant):
    """bdpt_test_alpha == oracle_alpha_test on every record of the mix that sits on a non-opaque triangle (the device keeps
    records for those only); an opaque triangle passes"""
    sc, lib, osc, b, ref = _world(pkg, ob)
    gpu_ctx.set_scene(sc.desc)
    masked = np.array([(m.flags >> 17) & 3 != 0 for m in sc.mats])[b.prim // 2]
    assert 0.3 * b.n < masked.sum() < b.n
    want = ob.alpha_test(pkg.abi, osc, b.prim.astype(np.uint32), b.uv)
    got = gpu_ctx.test_alpha(variant, b.prim, b.uv)
    assert not got[~masked].any()
    bad = (got != want) & masked
    assert not bad.any(), (variant, b.tally(bad))
    for name in es.ALPHA_FAMILIES + es.ADDRESS_FAMILIES:  # both verdicts occur in every family that can give both
        m = b.of(name) & masked
        assert want[m].any() and not want[m].all(), name


def test_alpha_hook_refuses_a_prim_outside_the_scene(pkg, ob, gpu_ctx):
    sc, lib, osc, b, ref = _world(pkg, ob)
    gpu_ctx.set_scene(sc.desc)
    with pytest.raises(pkg.BdptError):
        gpu_ctx.test_alpha(0, np.array([2 * sc.nq], np.uint32), np.zeros((1, 2), np.float32))
    with pytest.raises(pkg.BdptError):
        gpu_ctx.test_alpha(3, np.array([0], np.uint32), np.zeros((1, 2), np.float32))


def test_rays_straight_down_answer_like_the_scan(pkg, ob, gpu_ctx):
    """exact dyadic rays onto every quad (the alpha cards with their ties among them): bdpt_trace_rays in its three modes ==
    the oracle's tree == its linear scan == bdpt_test_trace, and the persistent any-hit kernel agrees on occlusion"""
    sc, lib, osc, b, ref = _world(pkg, ob)
    gpu_ctx.set_scene(sc.desc)
    rays = es.down_rays(sc)
    assert len(rays) < 10000
    for mode in MODES:
        prim = _check_all(gpu_ctx, lib, osc, rays, mode, len(rays))
        assert 0.2 * len(rays) < (prim >= 0).sum() < len(rays), mode  # some candidates are ignored, some culled
    occluded = _oracle(lib, osc, rays, "any", 1)[0] >= 0
    rays0 = rays.copy()
    assert (rays0[:, 6] == rays0[0, 6]).all()  # one tmin per launch
    vis, _ = gpu_ctx.test_trace_shadow(rays0)
    assert np.array_equal(vis == 0, occluded)
    # the closest hit's barycentrics are exact: x and y within the quad, dyadic
    hp, ht = _oracle(lib, osc, rays, "closest", 1)
    hit = hp >= 0
    x, y = rays[hit, 0] - 2 * (hp[hit] // 2), rays[hit, 1]
    on_a = hp[hit] % 2 == 0
    assert np.array_equal(ht[hit][on_a, 1], x[on_a]) and np.array_equal(ht[hit][on_a, 2], y[on_a])


@pytest.mark.parametrize("steps", [1, 2])
def test_walk_vertices_from_rays_straight_down(pkg, ob, gpu_ctx, steps):
    """bdpt_walk_query from the dyadic rays, on the finite quads under one large quad at z = 2 (the row alone is flat: a ray
    sampled at a first vertex would leave it): every real vertex, the second step's on the ceiling or back on the row
    included, is oracle_shade_hits (without the normal map) of the scan's closest hit of the ray that reached it, and a
    walk has a real vertex exactly where the scan has a hit."""
    import torch
    sc = es.EdgeScene(pkg.abi, finite=True, ceiling=True)
    lib = ob.load_oracle(pkg.abi)
    osc = lib.oracle_scene_create(C.byref(sc.desc))
    gpu_ctx.set_scene(sc.desc)
    rays = es.down_rays(sc)
    n = len(rays)
    starts = np.zeros((n, 12), np.float32)
    starts[:, 0:8], starts[:, 8:11] = _to_bdpt(rays), 1.0
    seeds = np.random.default_rng(3).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    samples = torch.zeros((steps, n, 8), dtype=torch.float32, device="cuda")
    hits = torch.zeros((steps, n, 4), dtype=torch.float32, device="cuda")
    vert, info = gpu_ctx.walk(_gpu(starts), _gpu(seeds), steps, mat_index=0, min_t=1e-4, samples=samples, hits=hits)
    torch.cuda.synchronize()
    vert, status = vert.cpu().numpy(), info.cpu().numpy().view(np.int32)[..., 3]
    samples, hits = samples.cpu().numpy(), hits.cpu().numpy()
    real = (status & pkg.abi.WALK_STATUS_REAL) != 0
    cur = rays
    for k in range(steps):
        hp, ht = _oracle(lib, osc, cur, "closest", 1)
        alive = real[k - 1] if k else np.ones(n, bool)
        assert np.array_equal(real[k], alive & (hp >= 0)), k
        m = real[k]
        assert m.sum() > 100, k
        oh = np.zeros((n, 4), np.float32)
        oh[:, 0:3] = ht
        oh.view(np.int32)[:, 3] = hp
        assert _same(hits[k][m], oh[m]).all(), k
        want = ob.shade_hits(pkg.abi, osc, _to_bdpt(cur), oh, 0)
        bad = ~_same(vert[k], want).all(axis=1) & m
        assert not bad.any(), (k, int(bad.sum()))
        nxt = np.zeros((n, 8), np.float32)  # the next ray: from the vertex along the sampled direction, tmin min_t
        nxt[:, 0:3], nxt[:, 3:6], nxt[:, 6], nxt[:, 7] = vert[k][:, 0:3], samples[k][:, 0:3], 1e-4, 1e38
        cur = np.where(m[:, None], nxt, cur)
    lib.oracle_scene_destroy(osc)


@pytest.mark.parametrize("view", ["start", "end"])
@pytest.mark.parametrize("mat_index", [0, 1], ids=["ggx", "lambert"])
def test_frames_of_the_finite_scene_bit_exact(pkg, ob, mat_index, view):
    """64 x 48, depth 4, on the quads whose shading is finite: the G-buffer channels (gbuffer_kernel with the normal map)
    and the image (walk_kernel with its LDS table, the any-hit kernel through the alpha cards) == oracle_gbuffer / oracle_bdpt.
    The "start" camera sees the normal-mapped quads, the "end" camera the addressing quads and alpha cards."""
    import torch
    sc = es.EdgeScene(pkg.abi, finite=True, view=view)
    pipe = pkg.FramePipeline(sc, 64, 48, max_depth=4, mat_index=mat_index)
    gp, p = pipe.render_frame()
    torch.cuda.synchronize()
    orc = ob.OracleRender(pkg.abi, sc.desc, 64, 48)
    orc.gbuffer(pipe.cam, gp)
    orc.bdpt(pipe.cam, p)
    for ch, on in (("MaterialDiffuse", "materialDiffuse"), ("MaterialSpecRough", "materialSpecRough"), ("Emissive", "emissive"),
                   ("WorldNormal", "worldNormal")):
        g = pipe.channels[ch].float().cpu().numpy().reshape(-1, 4)
        assert _same(g, orc.chan[on]).all(), ch
    orc.resolve()
    gpu, ref = pipe.output.cpu().numpy(), orc.image()
    assert np.isfinite(ref).all()
    assert np.array_equal(gpu.view(np.uint32), ref.view(np.uint32)), f"{(gpu != ref).any(axis=-1).sum()} pixels differ"
    assert (ref[..., :3] > 0).any(axis=-1).sum() > 500
    assert (orc.chan["worldPosition"][:, 3] != 0).sum() > 500
    orc.close()
    pipe.close()


def _always_fails(sc, k):
    """whether quad k's alpha test fails at every UV by the rule of the build's alpha clipping, which drops such triangles
    (bdpt_bvh_info.numDropped): a constant alpha below the threshold, or every texel more than 1e-5 below it"""
    m = sc.mats[k]
    if (m.flags >> 17) & 3 == 0:
        return False
    typ, thr = (m.flags >> 3) & 7, np.float32(m.alphaThreshold)
    if typ == 0:
        return bool(np.float32(0.0) < thr)
    if typ == 1 or m.texBaseColor < 0:
        return bool(np.float32(m.baseColor[3]) < thr)
    a = sc.textures[m.texBaseColor][0][..., 3]
    return bool(np.float32(a.max()) / np.float32(255.0) < thr - np.float32(1e-5))


def test_area_light_samples_on_the_alpha_cards(pkg, ob, gpu_ctx):
    """Every quad of the scene emits, the alpha cards with their ties among them: bdpt_test_area_light_sample ==
    oracle_area_light_sample in all 16 floats, modes 0 and 1 (Le = 0 where the alpha test fails at the sampled point).  The
    oracle is told which cards the build dropped: those whose test fails everywhere."""
    from area_scenes import oracle_exclude, oracle_info, oracle_sample
    sc, lib, _, b, ref = _world(pkg, ob)
    gpu_ctx.set_scene(sc.desc)
    dropped = [2 * k + t for k in range(sc.nq) if _always_fails(sc, k) for t in (0, 1)]
    assert 10 < len(dropped) < sc.nq and gpu_ctx.bvh_info().numDropped == len(dropped)
    osc = lib.oracle_scene_create(C.byref(sc.desc))
    oracle_exclude(lib, osc, dropped)
    o, g = oracle_info(pkg, lib, osc), gpu_ctx.area_light_info()
    assert (o.numEmitters, o.numTextured) == (g.numEmitters, g.numTextured) and o.numEmitters > sc.nq
    assert np.float32(o.totalWeight).view(np.uint32) == np.float32(g.totalWeight).view(np.uint32)
    rng = np.random.default_rng(9)
    n = 8192
    states = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    points = np.stack([rng.uniform(0, 2 * sc.nq, n), rng.uniform(-1, 2, n), rng.uniform(0.25, 3, n)], axis=1).astype(np.float32)
    for mode in (0, 1):
        want = oracle_sample(lib, osc, mode, states, points if mode else None)
        got = gpu_ctx.test_area_light_sample(mode, states, points if mode else None)
        bad = ~_same(got, want).all(axis=1)
        assert not bad.any(), (mode, int(bad.sum()))
        prim = want.view(np.uint32)[:, 0]
        le = want[:, 12:15] if mode == 0 else want[:, 5:8]
        masked = np.array([(m.flags >> 17) & 3 != 0 for m in sc.mats])[prim // 2]
        dark = (le == 0).all(axis=1)
        assert (dark & masked).sum() > 100 and (~dark & masked).sum() > 100, mode  # the test fails at some points and passes at others
    lib.oracle_scene_destroy(osc)


def test_occluder_hints_through_the_alpha_cards(pkg, ob, gpu_ctx):
    """bdpt_light_query NEE from points under the row toward the light above it: with BDPT_LIGHT_USE_HINTS the records equal
    those without hints but for the hint bit, and a ray the hint calls occluded (recOccludes: the hinted card's alpha test
    at the ray's own UV) is occluded for the oracle's linear scan too"""
    import torch
    sc, lib, osc, b, ref = _world(pkg, ob)
    gpu_ctx.set_scene(sc.desc)
    rng = np.random.default_rng(10)
    n = 8192
    surf = np.zeros((n, 24), np.float32)
    surf[:, 0], surf[:, 1], surf[:, 2] = rng.uniform(0, 2 * sc.nq, n), rng.uniform(0.05, 0.95, n), -rng.uniform(0.05, 0.5, n)
    surf[:, 6] = surf[:, 10] = 1.0
    surf[:, 7], surf[:, 12:15], surf[:, 16:19] = 0.5, 0.5, 0.25
    seeds = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.int32)
    plain = gpu_ctx.sample_lights(_gpu(surf), _gpu(seeds), mat_index=1, min_t=1e-4, use_hints=False)
    hinted = gpu_ctx.sample_lights(_gpu(surf), _gpu(seeds), mat_index=1, min_t=1e-4, use_hints=True)
    torch.cuda.synchronize()
    plain, hinted = plain.cpu().numpy(), hinted.cpu().numpy()
    bit = np.uint32(2 << 16)
    assert (plain.view(np.uint32)[:, 11] & bit == 0).all()
    called = hinted.view(np.uint32)[:, 11] & bit != 0
    h = hinted.copy()
    h.view(np.uint32)[:, 11] &= ~bit
    assert _same(h, plain).all()
    rays = np.concatenate([plain[:, 0:3], plain[:, 4:7], plain[:, 3:4], plain[:, 7:8]], axis=1)
    occluded = _oracle(lib, osc, rays, "any", 1)[0] >= 0
    assert called.sum() > 500 and not (called & ~occluded).any(), int((called & ~occluded).sum())
    print("hints: called occluded", int(called.sum()), "occluded for the scan", int(occluded.sum()), "of", n)
