"""GPU tests of MIS sky lighting (csrc/sky_mis.hip, bsdf_pdf_kernel of csrc/env_light.hip): bdpt_bsdf_pdf_query against
bdpt_bsdf_query's own pdf, a torch fp32 and a float64 reading of its formulas; bdpt_sky_mis_query and bdpt_sky_mis_execute
against the composed loop they replace (tests/sky_mis_reference.py), bit for bit — colour words, counts and states over every
item, both materials, every technique set — plus alive masks, device counts, tiles, capture, the error cases, the host pass
and unbiasedness against a float64 quadrature."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch  # (before the library is loaded: see tests/test_gpu_env.py)

import ao_reference as ar
import edge_records as er
import env_numpy as en
import sky_mis_reference as mr
from area_scenes import bits
from test_gpu_env import H, MIN_T, W, _records, bind, setup, words
from walk_loop import gpu, host

pytestmark = pytest.mark.gpu

F, U, D = np.float32, np.uint32, np.float64
FLT_MAX = float(en.FLT_MAX)
CLAMPS = (1.0, FLT_MAX)
DRAWS = {1: 4, 2: 3, 3: 7}  # draws per sample of a technique set
_state = {}


def _pdf(ctx, surf, dirs, mat, count=None, fill=-7):
    out = torch.full((len(surf), 4), float(fill), dtype=torch.float32, device="cuda")
    res = ctx.bsdf_pdf(gpu(np.ascontiguousarray(surf, F)), gpu(np.ascontiguousarray(dirs, F)), mat, out=out, count=count)
    assert res is out
    torch.cuda.synchronize()
    return host(out)


# ---- the density query -----------------------------------------------------------------------------------------------
def test_lambertian_density_is_the_samplers_own(pkg):
    """matIndex 1: pdf equals, bit for bit, the pdf bdpt_bsdf_query(SAMPLE) reports for the direction it drew; fcos equals
    (saturate(N.L) * diffuse) / kPi in torch fp32"""
    s = setup(pkg)
    ctx = s["ctx"]
    surf, seeds = _records(s)
    smp = host(ctx.sample_bsdf(gpu(surf), gpu(seeds.view(np.int32)), 1, False))
    dirs = np.ascontiguousarray(smp[:, 0:4])
    got = _pdf(ctx, surf, dirs, 1)
    lv = surf.view(np.int32)[:, 23] >= 0
    assert lv.sum() > 2000 and (~lv).sum() >= 64
    assert np.array_equal(words(got[lv, 3]), words(smp[lv, 3]))
    assert (got[lv, 3] > 0).sum() > 2000
    assert np.array_equal(words(got), words(mr.fcos_pdf_torch(surf, dirs, 1)))
    assert not got[~lv].view(U).any()


def _well_conditioned(n=2048, seed=21):
    """GGX records and directions with N.L, N.V and L.H at least 2^-4 and linearRoughness in [0.37, 1]"""
    rng = np.random.default_rng(seed)
    m = 8 * n
    Nn, V, L = er.unit(rng, m), er.unit(rng, m), er.unit(rng, m)
    dotf = lambda a, b: (a.astype(D) * b.astype(D)).sum(axis=1)
    Hh = V.astype(D) + L.astype(D)
    Hh /= np.linalg.norm(Hh, axis=1, keepdims=True)
    ok = (dotf(Nn, L) >= 0.0626) & (dotf(Nn, V) >= 0.0626) & ((L.astype(D) * Hh).sum(axis=1) >= 0.0626)
    keep = np.nonzero(ok)[0][:n]
    assert len(keep) == n
    surf = np.zeros((n, 24), F)
    surf[:, 4:7], surf[:, 8:11] = Nn[keep], V[keep]
    surf[:, 7] = rng.uniform(0.37, 1.0, n).astype(F)
    surf[:, 12:15], surf[:, 16:19] = rng.uniform(0.05, 1, (n, 3)).astype(F), rng.uniform(0.02, 1, (n, 3)).astype(F)
    dirs = np.zeros((n, 4), F)
    dirs[:, 0:3] = L[keep]
    return surf, dirs


def test_ggx_density_against_a_float64_reading(pkg):
    """matIndex 0 on well-conditioned records: fcos and pdf within 1e-4 relative (DESIGN section 2's bar for float64
    readings) of the formulas read in float64, every item.  There a2 = lr^4 >= 0.0178, so d >= a2 and d * d * pi is above the
    0.001 of ggxNormalDistribution's max: the clamp is inactive, and the cancellation in d costs about 2^-24 / 0.0178 = 3.4e-6
    on d, twice that on D."""
    s = setup(pkg)
    surf, dirs = _well_conditioned()
    fcos, pdf, q = mr.ggx_fcos_pdf_f64(surf, dirs)
    assert min(q["NdotL"].min(), q["NdotV"].min(), q["LdotH"].min()) >= 2.0 ** -4 and q["a2"].min() >= 0.0178 and q["d2pi"].min() > 0.001
    got = _pdf(s["ctx"], surf, dirs, 0).astype(D)
    rel_f = np.abs(got[:, 0:3] - fcos) / fcos
    rel_p = np.abs(got[:, 3] - pdf) / pdf
    print(f"GGX density, {len(surf)} items: worst relative error fcos {rel_f.max():.3e}, pdf {rel_p.max():.3e}")
    assert (fcos > 0).all() and (pdf > 0).all()
    assert (rel_f <= 1e-4).all() and (rel_p <= 1e-4).all(), (float(rel_f.max()), float(rel_p.max()))


def test_density_on_the_edge_families(pkg):
    """every record of tests/edge_records.py's BSDF families toward its L, both materials: the four words, a NaN equal to a
    NaN, against the formulas in torch fp32"""
    s = setup(pkg)
    mixed = er.bsdf_mixed()
    for mat in (1, 0):
        got = _pdf(s["ctx"], mixed.surf, mixed.dirs, mat)
        want = mr.fcos_pdf_torch(mixed.surf, mixed.dirs, mat)
        bad = (words(got) != words(want)).any(axis=1)
        assert not bad.any(), (mat, mixed.tally(bad))
        assert not got[mixed.prim < 0].view(U).any()
    assert np.isnan(got).any() and (got[:, 3] == 0).any() and (got[:, 3] > 0).any()


def test_density_device_count_capture_and_errors(pkg):
    """numDevice below, at and above num with the words beyond untouched; a capture holds one kernel node; the error cases
    in bdpt_bsdf_query's order"""
    from test_gpu_ao import _captured_once
    a = pkg.abi
    lib = pkg.load_library()
    s = setup(pkg)
    ctx = s["ctx"]
    surf, dirs = _well_conditioned(200, 5)
    n = len(surf)
    want = _pdf(ctx, surf, dirs, 0)
    for m in (0, 1, 63, 64, 65, n, n + 9):
        got = _pdf(ctx, surf, dirs, 0, count=torch.tensor([m], dtype=torch.int32, device="cuda"))
        k = min(m, n)
        assert np.array_equal(got[:k].view(U), want[:k].view(U)) and (got[k:] == -7.0).all(), m
    h = ctx.bsdf_pdf(surf, dirs, 0)  # host arrays go to the device and back
    assert isinstance(h, np.ndarray) and np.array_equal(h.view(U), want.view(U))
    st, dt, out = gpu(surf), gpu(dirs), torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    eager = _captured_once(lambda stream: ctx.bsdf_pdf(st, dt, 0, out=out, stream=stream), dict(out=out), [0])
    assert np.array_equal(host(eager["out"]).view(U), want.view(U))
    fresh = pkg.Context(0)
    out.fill_(-7)
    zeros = torch.zeros(4, dtype=torch.int32, device="cuda")
    P = dict(sf=st.data_ptr(), d=dt.data_ptr(), o=out.data_ptr(), n=zeros.data_ptr())

    def q(h=ctx._h, num=n, mat=0, flags=0, reserved=0, cnt=None, sf=P["sf"], d=P["d"], o=P["o"], desc=True):
        dd = a.BsdfPdfDesc()
        dd.num, dd.matIndex, dd.numDevice, dd.flags, dd.reserved, dd.surfaces, dd.dirs, dd.values = num, mat, cnt, flags, reserved, sf, d, o
        return lib.bdpt_bsdf_pdf_query(h, C.byref(dd) if desc else None, None)

    assert q(h=fresh._h) == -2 and b"bsdf_pdf_query" in lib.bdpt_last_error(fresh._h) and b"no scene" in lib.bdpt_last_error(fresh._h)
    assert q(h=fresh._h, mat=2) == -2  # the state comes first
    fresh.close()
    bad = [q(h=None), q(desc=False), q(mat=2), q(flags=1), q(reserved=1), q(num=0, mat=2), q(sf=None), q(sf=P["sf"] + 4), q(d=None),
           q(d=P["d"] + 8), q(o=None), q(o=P["o"] + 4), q(cnt=P["n"] + 2)]
    assert all(rc == -1 for rc in bad), bad
    assert q(num=0, sf=None, d=None, o=None) == 0
    torch.cuda.synchronize()
    assert (host(out) == -7).all()
    assert q(cnt=P["n"]) == 0 and q() == 0  # a device count of 0 writes nothing, then the whole call
    torch.cuda.synchronize()
    assert np.array_equal(host(out).view(U), want.view(U))


# ---- fused against the composed loop -----------------------------------------------------------------------------------
def _mis_records(s):
    """the Cornell items twice, with specular and roughness overridden so that both GGX lobes are drawn (linearRoughness 0.37
    with specular 0.04, 0.9 with 0.8), then the edge records and the non-finite positions of tests/test_gpu_env.py"""
    if "rec" not in _state:
        base, _ = _records(s)
        n0 = len(s["surf"])
        a, b = base[:n0].copy(), base[:n0].copy()
        a[:, 7], a[:, 16:19] = F(0.37), F(0.04)
        b[:, 7], b[:, 16:19] = F(0.9), F(0.8)
        surf = np.ascontiguousarray(np.concatenate([a, b, base[n0:]]))
        seeds = np.random.default_rng(12).integers(0, 2**32, len(surf), dtype=np.uint64).astype(U)
        _state["rec"] = (surf, seeds)
    return _state["rec"]


def _loop_of(s, name, mat, tech):
    """the composed loop's answers for map `name` (bound by the caller), once per (map, material, techniques) and shared:
    samples 1 and 2, and 64 for both techniques together; both clamps from one pass"""
    key = (name, mat, tech)
    if key not in _state:
        surf, seeds = _mis_records(s)
        _state[key] = mr.mis_loop(s["ctx"], surf, seeds, mat, tech, CLAMPS, (1, 2, 64) if tech == 3 else (1, 2), MIN_T)
    return _state[key]


def _assert_same(got, want, what):
    for name, g, w in zip(("color", "counts", "seeds_out"), got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        diff = g.view(U) != w.view(U)
        assert not diff.any(), (f"{what}: {name} differ in {int(diff.sum())} of {diff.size} words, first item "
                                f"{int(np.argmax(diff.reshape(len(g), -1).any(axis=1)))}")


@pytest.mark.parametrize("mat", [1, 0])
@pytest.mark.parametrize("name", ["sun", "7x5"])
def test_equals_the_composed_loop(pkg, name, mat):
    """techniques 1, 2 and 3 at samples 1 and 2, and 64 for techniques 3; clampUpper 1 and FLT_MAX: colour words, counts and
    states of every item equal the loop's"""
    s = setup(pkg)
    ctx = s["ctx"]
    surf, seeds = _mis_records(s)
    keep = bind(ctx, s["maps"][name][0])
    lv = surf.view(np.int32)[:, 23] >= 0
    if mat == 0:  # both lobes are drawn
        lobe = host(ctx.sample_bsdf(gpu(surf), gpu(seeds.view(np.int32)), 0, True)).view(U)[lv, 7]
        assert (lobe == 0).sum() > 500 and (lobe == 1).sum() > 500
    for tech in (1, 2, 3):
        want, traced = _loop_of(s, name, mat, tech)
        for clamp in CLAMPS:
            for samples in ((1, 2, 64) if tech == 3 else (1, 2)):
                got = mr.mis_query(ctx, surf, seeds, samples, mat, tech, clamp, MIN_T)
                _assert_same(got, want[(clamp, samples)], f"{name} mat {mat} techniques {tech} S {samples} clamp {clamp}")
                color, counts, sout = got
                assert np.array_equal(color[~lv, 0:3].view(U), surf[~lv, 12:15].view(U)) and (counts[~lv] == 0).all()
                assert np.array_equal(sout[~lv], seeds[~lv]) and np.array_equal(sout[lv], en.draws(seeds[lv], DRAWS[tech] * samples)[1])
                assert (color[:, 3] == 1.0).all() and (counts <= (2 if tech == 3 else 1) * samples).all()
                if clamp == 1.0:
                    assert (color[lv, 0:3] <= (2.0 if tech == 3 else 1.0)).all()
        last = want[(FLT_MAX, 64 if tech == 3 else 2)][1]
        assert (last[lv] > 0).any() and (last[lv] < traced[lv]).any(), tech  # lit and shadowed terms both occur
    if name == "sun":
        w = _loop_of(s, name, mat, 3)[0]
        assert not np.array_equal(w[(1.0, 64)][0], w[(FLT_MAX, 64)][0])  # the clamp bites
    del keep
    ctx.set_environment()


def test_alive_masks_device_counts_and_item_counts(pkg):
    """alive bytes that drop every third item; device counts below, at and above num with the words beyond untouched; 1, 63,
    64, 65 items; seeds_out in place; host arrays"""
    s = setup(pkg)
    ctx = s["ctx"]
    surf, seeds = _mis_records(s)
    keep = bind(ctx, s["maps"]["7x5"][0])
    n, S, mat, tech = len(surf), 2, 0, 3
    want = _loop_of(s, "7x5", mat, tech)[0][(FLT_MAX, S)]
    for m in (1, 63, 64, 65):
        _assert_same(mr.mis_query(ctx, surf[:m], seeds[:m], S, mat, tech, FLT_MAX, MIN_T), [w[:m] for w in want], f"{m} items")
    for m in (0, 1, 63, 64, 65, n, n + 9):
        cnt = torch.tensor([m], dtype=torch.int32, device="cuda")
        got = mr.mis_query(ctx, surf, seeds, S, mat, tech, FLT_MAX, MIN_T, count=cnt)
        k = min(m, n)
        _assert_same([g[:k] for g in got], [w[:k] for w in want], f"device count {m}")
        assert (got[0][k:] == -7.0).all() and (got[1].view(np.int32)[k:] == -7).all() and (got[2].view(np.int32)[k:] == -7).all(), m
    alive = (np.arange(n) % 3 != 1).astype(np.uint8)
    got = mr.mis_query(ctx, surf, seeds, S, mat, tech, FLT_MAX, MIN_T, alive=alive)
    _assert_same(got, mr.mis_loop(ctx, surf, seeds, mat, tech, (FLT_MAX,), (S,), MIN_T, alive=alive)[0][(FLT_MAX, S)], "alive")
    dead = alive == 0
    assert np.array_equal(got[0][dead, 0:3].view(U), surf[dead, 12:15].view(U)) and (got[1][dead] == 0).all()
    assert np.array_equal(got[2][dead], seeds[dead])
    st = gpu(seeds.view(np.int32))
    ctx.sky_lighting_mis(gpu(surf), st, S, mat_index=mat, min_t=MIN_T, seeds_out=st)
    torch.cuda.synchronize()
    assert np.array_equal(host(st).view(U), want[2])
    h = ctx.sky_lighting_mis(surf[:65], seeds[:65], S, mat_index=mat, min_t=MIN_T)
    assert isinstance(h, np.ndarray) and np.array_equal(h.view(U), want[0][:65].view(U))
    del keep
    ctx.set_environment()


def test_all_zero_map(pkg):
    """total == 0: colour 0, every draw taken, no term counted, for every technique set and both materials"""
    s = setup(pkg)
    ctx = s["ctx"]
    surf, seeds = _mis_records(s)
    keep = bind(ctx, s["maps"]["zero"][0])
    lv = surf.view(np.int32)[:, 23] >= 0
    for mat in (1, 0):
        for tech in (1, 2, 3):
            for samples in (1, 64):
                color, counts, sout = mr.mis_query(ctx, surf, seeds, samples, mat, tech, FLT_MAX, MIN_T)
                assert not color[lv, 0:3].view(U).any() and (color[:, 3] == 1.0).all() and not counts.any()
                assert np.array_equal(sout[lv], en.draws(seeds[lv], DRAWS[tech] * samples)[1]) and np.array_equal(sout[~lv], seeds[~lv])
    del keep
    ctx.set_environment()


# ---- the pass ------------------------------------------------------------------------------------------------------------
def _gbuffer_records(pipe, frame, mat):
    """the query's inputs for the pass: positions, half-decoded normals and diffuse, prim from worldPosition.w, the pass's
    seeds; for GGX also specular and linearRoughness from MaterialSpecRough and V = normalize(camera - posW) in fp32"""
    from test_gpu_sky import _gbuffer_records as plain
    rec, seeds = plain(pipe, frame)
    if mat == 0:
        sr = host(pipe.channels["MaterialSpecRough"].float()).reshape(-1, 4)
        rec[:, 16:19], rec[:, 7] = sr[:, 0:3], sr[:, 3]
        with np.errstate(all="ignore"):
            d = (np.array(list(pipe.cam.posW), F)[None, :] - rec[:, 0:3]).astype(F)
            inv = (F(1.0) / np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F) + d[:, 2] * d[:, 2]).astype(F)).astype(F)).astype(F)
            rec[:, 8:11] = (d * inv[:, None]).astype(F)
    return rec, seeds


@pytest.mark.parametrize("mat", [1, 0])
def test_execute_equals_the_query_and_tiles_reproduce_the_frame(pkg, mat):
    """bdpt_sky_mis_execute equals the query fed the G-buffer; two row tiles and a stripes context write only their pixels,
    with the whole frame's values; the frame counter advances by one per call and is the plain pass's"""
    s = setup(pkg)
    pipe, ctx, a = s["pipe"], s["ctx"], pkg.abi
    env_t = bind(ctx, s["maps"]["7x5"][0])
    st = pipe._stream_ptr()
    ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, st)
    torch.cuda.synchronize()
    S, clamp = 4, 2.0
    images = {}
    for frame in (0, 0, 5):
        pipe.sky_frame = frame
        img = host(pipe.sky_lighting(S, clamp, mis=True, mat_index=mat)).copy()
        p = pipe.last_sky_params
        assert pipe.sky_frame == frame + 1 and (p.frameCount, p.matIndex, p.techniques, p.samples) == (frame, mat, 3, S)
        if frame in images:
            assert np.array_equal(bits(img), bits(images[frame]))
        images[frame] = img
    assert not np.array_equal(bits(images[0]), bits(images[5]))
    for frame, img in images.items():
        rec, seeds = _gbuffer_records(pipe, frame, mat)
        color, _, _ = mr.mis_query(ctx, rec, seeds, S, mat, 3, clamp, MIN_T)
        assert np.array_equal(bits(img), bits(color.reshape(H, W, 4))), frame
        background = rec.view(np.int32)[:, 23] < 0
        assert background.any() and (color[~background, 0:3] > 0).any()
    p = a.SkyMisParams(0, clamp, MIN_T, S, mat, 3)
    for kind, args in (("rows", (0, 16)), ("rows", (16, H)), ("stripes", None)):
        tile = pkg.Context(0)
        tile.set_scene(s["scene"].desc)
        if kind == "rows":
            tile.resize(W, H, args[0], args[1], 3)
        else:
            tile.resize_stripes(W, H, 4, 3, 1, 3)
        tile.set_environment(env_t.data_ptr(), 7, 5)
        tile.env_prepare()
        if mat == 0:
            tile.set_camera(pipe.cam)
        rows = np.zeros(H, bool)
        for y0, y1 in tile.row_ranges():
            rows[y0:y1] = True
        assert 0 < rows.sum() < H
        out = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
        tile.sky_mis_execute(p, pipe.gb, C.c_void_p(out.data_ptr()), st)
        torch.cuda.synchronize()
        got = host(out)
        assert np.array_equal(bits(got[rows]), bits(images[0][rows])), kind
        assert (got[~rows] == -7.0).all(), kind
        tile.close()
    pipe.sky_frame = 0
    ctx.set_environment()


def test_captured_query_and_execute(pkg):
    """bdpt_sky_mis_query and bdpt_sky_mis_execute captured: each graph holds exactly one kernel node, capturing allocates
    nothing, and two replays equal the eager call"""
    from test_gpu_ao import _captured_once
    s = setup(pkg)
    pipe, ctx = s["pipe"], s["ctx"]
    keep = bind(ctx, s["maps"]["7x5"][0])
    ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, pipe._stream_ptr())
    torch.cuda.synchronize()
    img = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    p = pkg.abi.SkyMisParams(3, FLT_MAX, MIN_T, 4, 0, 3)
    eager = _captured_once(lambda st: ctx.sky_mis_execute(p, pipe.gb, C.c_void_p(img.data_ptr()), st), dict(img=img), [0])
    rec, seeds = _gbuffer_records(pipe, 3, 0)
    color, counts, sout = mr.mis_query(ctx, rec, seeds, 4, 0, 3, FLT_MAX, MIN_T)
    assert np.array_equal(bits(host(eager["img"])), bits(color.reshape(H, W, 4)))
    n = len(rec)
    rt, sd = gpu(rec), gpu(seeds.view(np.int32))
    outs = dict(col=torch.zeros((n, 4), dtype=torch.float32, device="cuda"), c=torch.zeros(n, dtype=torch.int32, device="cuda"),
                so=torch.zeros(n, dtype=torch.int32, device="cuda"))
    eager = _captured_once(lambda st: ctx.sky_lighting_mis(rt, sd, 4, mat_index=0, techniques=3, min_t=MIN_T, out=outs["col"], counts=outs["c"],
                                                           seeds_out=outs["so"], stream=st), outs, [0])
    assert np.array_equal(bits(host(eager["col"])), bits(color)) and np.array_equal(host(eager["c"]).view(U), counts)
    assert np.array_equal(host(eager["so"]).view(U), sout)
    del keep
    ctx.set_environment()


def test_error_cases_through_the_c_abi(pkg):
    """every error case in the documented order, nothing enqueued: no scene, no size, no map, a stale table, no camera for
    matIndex 0, samples 0 and 65, matIndex 2, techniques 0 and 4, flags, reserved, misaligned buffers"""
    a = pkg.abi
    lib = pkg.load_library()
    s = setup(pkg)
    ctx = pkg.Context(0)
    n = 256
    surf = torch.zeros((n, 24), dtype=torch.float32, device="cuda")
    seeds = torch.zeros(n, dtype=torch.int32, device="cuda")
    alive = torch.ones(n, dtype=torch.uint8, device="cuda")
    cnt = torch.full((4,), n, dtype=torch.int32, device="cuda")
    col = torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda")
    outs = {k: torch.full((n,), -7, dtype=torch.int32, device="cuda") for k in ("c", "so")}
    img = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
    gpos = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    gh = torch.zeros((3, H, W, 4), dtype=torch.float16, device="cuda")
    env = gpu(en.random_map(7, 5, 4))
    P = dict(sf=surf.data_ptr(), sd=seeds.data_ptr(), b=alive.data_ptr(), n=cnt.data_ptr(), col=col.data_ptr(), img=img.data_ptr(),
             gp=gpos.data_ptr(), gn=gh[0].data_ptr(), gd=gh[1].data_ptr(), gs=gh[2].data_ptr(), **{k: t.data_ptr() for k, t in outs.items()})

    def q(h=ctx._h, num=n, samples=4, mat=0, tech=3, cnt=None, flags=0, reserved=0, sf=P["sf"], sd=P["sd"], al=None, color=P["col"], c=None,
          so=None, desc=True):
        d = a.SkyMisDesc()
        d.num, d.samples, d.numDevice, d.clampUpper, d.minT, d.flags, d.reserved = num, samples, cnt, 10.0, 1e-4, flags, reserved
        d.matIndex, d.techniques = mat, tech
        d.surfaces, d.seeds, d.alive, d.color, d.counts, d.seedsOut = sf, sd, al, color, c, so
        return lib.bdpt_sky_mis_query(h, C.byref(d) if desc else None, None)

    def x(h=ctx._h, samples=4, mat=0, tech=3, reserved=(0, 0), gp=P["gp"], gn=P["gn"], gd=P["gd"], gs=P["gs"], out=P["img"], params=True,
          gbuffer=True):
        p = a.SkyMisParams(0, 10.0, 1e-4, samples, mat, tech, (C.c_uint32 * 2)(*reserved))
        gb = a.GBuffer()
        gb.worldPosition, gb.worldNormal, gb.materialDiffuse, gb.materialSpecRough = gp, gn, gd, gs
        return lib.bdpt_sky_mis_execute(h, C.byref(p) if params else None, C.byref(gb) if gbuffer else None, out, None)

    err = lambda: lib.bdpt_last_error(ctx._h)
    assert q() == -2 and b"sky_mis_query" in err() and b"no scene" in err()
    assert x() == -2 and b"sky_mis_execute" in err()
    ctx.set_scene(s["scene"].desc)
    assert q() == -2 and b"no environment map" in err()  # a scene, but no map
    assert q(samples=0) == -2 and q(tech=0) == -2  # the state comes first
    assert x() == -2 and b"no size" in err()
    ctx.resize(W, H, 0, H, 3)
    assert x() == -2 and b"no environment map" in err()
    ctx.set_environment(env.data_ptr(), 7, 5)
    assert q() == -2 and x() == -2 and b"bdpt_env_prepare first" in err()  # a map, but no table
    ctx.env_prepare()
    ctx.set_environment(env.data_ptr(), 7, 5)  # the table goes stale with a new environment, even the same one
    assert q() == -2 and x(samples=0) == -2
    ctx.env_prepare()
    assert x() == -2 and b"no camera" in err() and x(samples=0) == -2  # matIndex 0 reads V from the camera: state before arguments
    assert x(mat=1, samples=0) == -1  # the Lambertian pass needs none
    ctx.set_camera(s["pipe"].cam)
    bad = [
        q(h=None), q(desc=False), q(samples=0), q(samples=65), q(samples=2**31), q(mat=2), q(tech=0), q(tech=4), q(tech=2**31), q(flags=1),
        q(reserved=1), q(num=0, samples=0), q(num=0, tech=0), q(sf=None), q(sf=P["sf"] + 4), q(sd=None), q(sd=P["sd"] + 2), q(color=None),
        q(color=P["col"] + 8), q(c=P["c"] + 1), q(so=P["so"] + 2), q(cnt=P["n"] + 2),
        x(h=None), x(params=False), x(gbuffer=False), x(samples=0), x(samples=65), x(mat=2), x(tech=0), x(tech=4), x(reserved=(1, 0)),
        x(reserved=(0, 1)), x(gp=None), x(gp=P["gp"] + 8), x(gn=None), x(gn=P["gn"] + 4), x(gd=None), x(gd=P["gd"] + 4), x(gs=None),
        x(gs=P["gs"] + 4), x(out=None), x(out=P["img"] + 8),
    ]
    assert all(rc == -1 for rc in bad), bad
    assert q(num=0, sf=None, sd=None, color=None) == 0
    torch.cuda.synchronize()
    for t in list(outs.values()) + [col, img]:
        assert (host(t) == -7).all()
    # and the good calls: every record at the origin with N = 0 has N.L = 0, so colour 0 after its draws (the GGX sampler's
    # direction has dot(N, L) <= 0: pdf 0, no term); a zero worldPosition.w is the background, which takes the (zero) diffuse
    assert q(al=P["b"], c=P["c"], so=P["so"], cnt=P["n"]) == 0 and q(mat=1, tech=1) == 0 and x() == 0
    assert x(mat=1, gs=None) == 0  # the Lambertian pass does not read MaterialSpecRough
    torch.cuda.synchronize()
    assert (host(col) == np.array([0, 0, 0, 1], F)).all() and (host(outs["c"]) == 0).all()
    assert (host(outs["so"]).view(U) == en.draws(np.zeros(1, U), 28)[1][0]).all()
    assert (host(img) == np.array([0, 0, 0, 1], F)).all()
    ctx.close()


def test_cpp_host_sky_mis_equals_the_python_pipeline(pkg, tmp_path):
    """bdpt_render --env probe.hdr --sky 4 --sky-mis --sky-ggx --raw on the Cornell box at 64 x 36, frame 0, equals
    FramePipeline.sky_lighting(4, mis=True, mat_index=0) under the same probe; and without --sky-ggx the Lambertian call"""
    import __graft_entry__ as ge
    from test_gpu_sky import _write_hdr
    exe = os.path.join(ge.PKG_DIR, "host", "bdpt_render")
    assert os.path.exists(exe), "host/bdpt_render not built (run __graft_entry__.build())"
    w, h = 64, 36
    probe = tmp_path / "probe.hdr"
    env = _write_hdr(pkg, probe, 16, 8)
    scene = pkg.Scene.cornell()
    pipe = pkg.FramePipeline(scene, w, h)
    t = gpu(env)
    pipe.ctx.set_environment(t.data_ptr(), 16, 8)
    gp = pipe.gbuffer_params()
    gp.envMap, gp.envWidth, gp.envHeight = t.data_ptr(), 16, 8
    pipe.ctx.gbuffer_execute(gp, pipe.gb, pipe._stream_ptr())
    images = []
    for extra, mat in ((["--sky-mis", "--sky-ggx"], 0), (["--sky-mis"], 1)):
        raw = tmp_path / f"sky{mat}.f32"
        r = subprocess.run([exe, "--scene", "cornell", "--width", str(w), "--height", str(h), "--frames", "1", "--env", str(probe), "--sky", "4"] +
                           extra + ["--out", str(tmp_path / "sky.pfm"), "--raw", str(raw)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        cpp = np.fromfile(raw, F).reshape(h, w, 4)
        pipe.sky_frame = 0
        img = host(pipe.sky_lighting(4, mis=True, mat_index=mat)).copy()
        assert pipe.last_sky_params.frameCount == 0
        assert np.array_equal(bits(cpp), bits(img)), mat
        assert (cpp[..., 3] == 1.0).all() and (cpp[..., 0:3] > 0).any()
        images.append(cpp)
    assert not np.array_equal(bits(images[0]), bits(images[1]))
    pipe.close()
    scene.close()


# ---- unbiasedness --------------------------------------------------------------------------------------------------------
def _estimates(ctx, rec, seeds, mat):
    out = {}
    for tech in (1, 2, 3):
        color, counts, _ = mr.mis_query(ctx, rec, seeds, 64, mat, tech, FLT_MAX, MIN_T)
        assert (counts > 0).all()
        est = color[:, 0:3].astype(D)
        out[tech] = (est.mean(axis=0), est.std(axis=0, ddof=1) / math.sqrt(len(rec)), est.var(axis=0, ddof=1))
    print("sample variance of a 64-sample estimate: " + ", ".join(f"techniques {t}: {v[2]}" for t, v in out.items()))
    return out


def _item_above_the_box(n=256):
    rec = ar.surface_records(np.tile(np.array([[278.0, 700.0, 280.0]], F), (n, 1)), np.tile(np.array([[0, 1, 0]], F), (n, 1)))
    seeds = np.random.default_rng(77).integers(0, 2**32, n, dtype=np.uint64).astype(U)
    return rec, seeds


def test_lambertian_converges_to_the_float64_quadrature(pkg):
    """an unoccluded upward-facing white item above the box under the 7 x 5 map, 64 samples x 256 seeds: with table samples,
    BSDF samples and both, the mean lies within 5 standard errors (from the 256 estimates themselves) of sum over texels
    radiance * integral of cos / pi over the texel"""
    s = setup(pkg)
    ctx = s["ctx"]
    env = s["maps"]["7x5"][0]
    keep = bind(ctx, env)
    rec, seeds = _item_above_the_box()
    rec[:, 12:15] = 1.0
    hh, ww = env.shape[:2]
    th0, th1 = np.pi * np.arange(hh) / hh, np.pi * (np.arange(hh) + 1) / hh
    th0, th1 = np.minimum(th0, np.pi / 2), np.minimum(th1, np.pi / 2)  # N = +y: the upper hemisphere
    weight = (np.sin(th1) ** 2 - np.sin(th0) ** 2) / ww  # integral of cos(theta) / pi over a texel of row y
    want = (env[..., :3].astype(D) * weight[:, None, None]).sum(axis=(0, 1))
    for tech, (mean, sem, _) in _estimates(ctx, rec, seeds, 1).items():
        print(f"techniques {tech}: quadrature {want}, mean {mean}, standard error {sem}")
        assert (sem > 0).all() and (np.abs(mean - want) <= 5 * sem).all(), (tech, mean, want, sem)
    del keep
    ctx.set_environment()


def test_ggx_technique_sets_agree(pkg):
    """the same item as a GGX surface (linearRoughness 0.6, V 45 degrees off N): the means with table samples, BSDF samples
    and both agree pairwise within 5 combined standard errors"""
    s = setup(pkg)
    ctx = s["ctx"]
    keep = bind(ctx, s["maps"]["7x5"][0])
    rec, seeds = _item_above_the_box()
    rec[:, 7], rec[:, 8:11] = F(0.6), np.array([math.sqrt(0.5), math.sqrt(0.5), 0.0], F)
    rec[:, 12:15], rec[:, 16:19] = F(0.5), F(0.5)
    est = _estimates(ctx, rec, seeds, 0)
    for a_, b_ in ((1, 2), (1, 3), (2, 3)):
        (ma, sa, _), (mb, sb, _) = est[a_], est[b_]
        both = np.sqrt(sa * sa + sb * sb)
        print(f"techniques {a_} vs {b_}: means {ma} {mb}, combined standard error {both}")
        assert (both > 0).all() and (np.abs(ma - mb) <= 5 * both).all(), (a_, b_, ma, mb, both)
    del keep
    ctx.set_environment()
