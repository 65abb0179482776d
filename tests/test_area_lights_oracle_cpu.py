"""CPU checks of the oracle's area lights (oracle/bdpt_oracle.cpp after include/bdpt.h "Area lights"): its emitter table
and its sampling hook against the float64 restatement (area_light_numpy.py), and its frames under the switch against the
float64 reading of the ray-generation shader (hlsl_integrator_numpy.py)."""
import ctypes as C
import math

import numpy as np
import pytest

from area_light_numpy import AREA_KEY, CHANNEL_TEXTURE, emissive_type
from area_scenes import (AREA, MIS_POWER, NO_CONNECT, NO_NEE, NO_SPLAT, AreaScene, emitter_soup, oracle_exclude,
                         oracle_info, oracle_sample, oracle_table)
from hlsl_integrator_numpy import hm_init_rand
from hlsl_reference_math import next_rand


@pytest.fixture(scope="module")
def cornell(pkg):
    s = pkg.Scene.cornell()
    yield s
    s.close()


def _pick32(cdf32, last, a):
    """the fp32 selection rule: binary search for the first CDF value > a * W, else the last emitter with w > 0"""
    target = np.float32(a) * cdf32[-1]
    lo, hi = 0, len(cdf32)
    while lo < hi:
        mid = (lo + hi) >> 1
        if cdf32[mid] > target:
            hi = mid
        else:
            lo = mid + 1
    return lo if lo < len(cdf32) else last


def _check_samples(tab, cdf32, last32, prim, states, pts, out0, out1):
    """The oracle's samples (out0: light start, out1: NEE) against the float64 restatement, with the tolerances of the
    GPU hook test; the pick itself against the fp32 rule exactly.  Returns how many samples were compared."""
    u32 = lambda x: x.view(np.uint32)
    checked = 0
    for k in range(len(states)):
        s, a = next_rand(int(states[k]))
        i32 = _pick32(cdf32, last32, a)
        assert int(u32(out0[k, 0:1])[0]) == prim[i32], k
        _, an = next_rand(hm_init_rand(int(states[k]), AREA_KEY))
        in32 = _pick32(cdf32, last32, an)
        assert int(u32(out1[k, 0:1])[0]) == prim[in32], k
        x, nrm, dirv, col, seed = tab.light_start(int(states[k]))
        assert int(u32(out0[k, 15:16])[0]) == seed
        if x["i"] != i32 or (x["alpha"] is not None and abs(x["alpha"][0] - x["alpha"][1]) < 1e-4) or tab.area[x["i"]] == 0:
            continue  # fp32 and float64 fall on different sides of a CDF boundary or of the alpha threshold
        g = out0[k]
        assert np.allclose(g[1:3], [x["b1"], x["b2"]], rtol=1e-4, atol=1e-5)
        assert np.allclose(g[3:6], x["pos"], rtol=1e-4, atol=1e-3)
        assert np.allclose(g[6:9], nrm, atol=1e-5)
        assert np.allclose(g[9:12], dirv, atol=2e-4)
        assert np.allclose(g[12:15], col, rtol=1e-4, atol=1e-6 * max(1.0, float(np.abs(col).max())))
        xn, L, d, inten = tab.nee(int(states[k]), pts[k].astype(np.float64))
        if xn["i"] != in32 or (xn["alpha"] is not None and abs(xn["alpha"][0] - xn["alpha"][1]) < 1e-4) or tab.area[xn["i"]] == 0:
            continue
        checked += 1
        h = out1[k]
        if d < 5.0:
            continue  # (fp32 positions put ~3e-5 into x - pos: within 5 units that exceeds 1e-4 of d^2)
        assert np.allclose(h[1:4], L, atol=1e-4) and math.isclose(h[4], d, rel_tol=1e-4)
        scale = float(np.abs(xn["Le"]).max()) / (xn["pA"] * d * d)
        assert np.allclose(h[5:8], inten, rtol=1e-4, atol=1e-5 * scale), k
        assert np.allclose(h[8:10], [xn["b1"], xn["b2"]], rtol=1e-4, atol=1e-5)
    return checked


@pytest.mark.parametrize("n", [6, 65, 5000])
def test_oracle_table_and_samples_match_float64_restatement(pkg, ob, cornell, n):
    """Emitter and textured counts equal; each weight within 1e-5 relative; every CDF value within n 2^-23 W of the
    float64 prefix sum; the pick exactly the fp32 rule; point, side, direction, colour and NEE intensity as the GPU hook
    test requires of the device."""
    sc = AreaScene(pkg, cornell) if n == 6 else emitter_soup(pkg, n, seed=n)
    lib = ob.load_oracle(pkg.abi)
    osc = lib.oracle_scene_create(C.byref(sc.desc))
    tab = sc.table()
    info = oracle_info(pkg, lib, osc)
    prim, w, ar, cdf = oracle_table(lib, osc)
    m = len(prim)
    assert info.numEmitters == m == len(tab.prim) and m >= n
    n_tex = sum(1 for t in tab.prim if emissive_type(sc.mats[int(sc.M[t])].flags) == CHANNEL_TEXTURE)
    assert info.numTextured == n_tex and n_tex > 0
    assert np.array_equal(prim, tab.prim)
    assert np.allclose(w, tab.w, rtol=1e-5, atol=0) and np.allclose(ar, tab.area, rtol=1e-5, atol=0)
    assert (np.abs(cdf.astype(np.float64) - tab.cdf) <= m * 2.0 ** -23 * tab.W).all()
    assert info.totalWeight == cdf[-1] and math.isclose(info.totalWeight, tab.W, rel_tol=1e-5)
    if n > 6:
        assert (w == 0).sum() >= 8 and w[-8:].max() == 0  # zero-area emitters, and a run of them at the end
    last32 = int(np.nonzero(w > 0)[0][-1])
    rng = np.random.default_rng(n)
    k = 3000
    states = rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32)
    lo, hi = sc.P.min(axis=0), sc.P.max(axis=0)
    pts = rng.uniform(lo, hi, (k, 3)).astype(np.float32)
    out0 = oracle_sample(lib, osc, 0, states)
    out1 = oracle_sample(lib, osc, 1, states, pts)
    checked = _check_samples(tab, cdf, last32, prim, states, pts, out0, out1)
    assert checked > 0.9 * k, checked
    lib.oracle_scene_destroy(osc)


def test_oracle_switch_changes_nothing_without_emitters_and_refuses_mis(pkg, ob, cornell):
    """No emitter: the frame with the switch is the frame without it, bit for bit; with MIS oracle_bdpt fails, as
    bdpt_execute does.  An excluded emitter leaves the table (oracle_area_exclude)."""
    from test_oracle_cross_check import _frame_params
    A = pkg.abi
    dark = AreaScene(pkg, cornell, patch_emission=(0.0, 0.0, 0.0), extra=False, point_light=True)
    # emitters that all have zero area: W == 0, which changes nothing either
    base = AreaScene(pkg, cornell, extra=False, point_light=True)
    P = base.P.copy()
    patch_v = np.unique(base.I[base.M == 3])
    P[patch_v] = P[patch_v[0]]
    flat = AreaScene(pkg, cornell, extra=False, point_light=True, positions=P)
    for sc in (dark, flat):
        imgs = []
        for flags in (0, AREA):
            gp, p = _frame_params(pkg, 4, 0, flags, 1e-4)
            orc = ob.OracleRender(A, sc.desc, 24, 24)
            info = oracle_info(pkg, orc.lib, orc.scene)
            assert info.numEmitters == len(sc.table().prim) and info.totalWeight == 0.0
            orc.gbuffer(sc.camera(1.0), gp)
            orc.bdpt(sc.camera(1.0), p)
            orc.resolve()
            imgs.append((orc.image().copy(), orc.splat.copy()))
            orc.close()
        assert np.array_equal(imgs[0][0].view(np.uint32), imgs[1][0].view(np.uint32)) and np.array_equal(imgs[0][1], imgs[1][1])
    assert len(flat.table().prim) > 0
    sc = AreaScene(pkg, cornell, point_light=True)
    orc = ob.OracleRender(A, sc.desc, 8, 8)
    gp, p = _frame_params(pkg, 3, 0, AREA | MIS_POWER, 1e-4)
    orc.gbuffer(sc.camera(1.0), gp)
    cnt = A.Counters()
    assert orc.lib.oracle_bdpt(orc.scene, C.byref(sc.camera(1.0)), C.byref(p), C.byref(orc.frame), 0, 1, C.byref(cnt)) == -1
    n0 = oracle_info(pkg, orc.lib, orc.scene).numEmitters
    patch = np.nonzero(sc.M == 3)[0]
    oracle_exclude(orc.lib, orc.scene, patch)
    assert oracle_info(pkg, orc.lib, orc.scene).numEmitters == n0 - len(patch)
    out_of_range = np.array([10 ** 6], np.uint32)
    assert orc.lib.oracle_area_exclude(orc.scene, out_of_range.ctypes.data, 1) == -1
    orc.close()


@pytest.mark.parametrize("size,depth,mat", [(16, 3, 1), (12, 4, 0)])
def test_area_light_frames_match_float64_reading_of_the_raygen_shader(pkg, ob, cornell, size, depth, mat):
    """test_integrator_matches_float64_reading_of_the_raygen_shader with the switch: the Cornell box with three constant
    emitters (the ceiling patch and two of other luminances, the floor seeing one from its back) beside its point light,
    all four sharing the numLights + 1 choice.  The float64 reading takes the table as light numLights
    (hlsl_integrator_numpy.Renderer(area=...)).  gMinT = 0.05 and ORACLE_CONNECT_ALL_VISIBLE as there; pixels may differ
    only where fp32 and float64 fall on different sides of a CDF boundary or a shadow edge: a small share."""
    import hlsl_integrator_numpy as hi
    from test_oracle_cross_check import _frame_params
    A = pkg.abi
    sc = AreaScene(pkg, cornell, extra=False, const_extra=True, point_light=True)
    tab = sc.table()
    assert len(tab.prim) == 6 and tab.W > 0
    cam = sc.camera(1.0)
    stages = (("nee", NO_SPLAT | NO_CONNECT, dict(splat=False, connect=False), 0),
              ("splat", NO_NEE | NO_CONNECT, dict(nee=False, connect=False), 0),
              ("connect", NO_NEE | NO_SPLAT, dict(nee=False, splat=False, connect_all_visible=True), ob.ORACLE_CONNECT_ALL_VISIBLE))
    for name, flags, kw, oflags in stages:
        gp, p = _frame_params(pkg, depth, mat, flags | AREA, 0.05)
        orc = ob.OracleRender(A, sc.desc, size, size)
        orc.gbuffer(cam, gp)
        orc.bdpt(cam, p, flags=oflags)
        own = orc.image().astype(np.float64)
        splat = orc.splat.astype(np.float64)
        splat[:, :3] /= 2.0 ** 32
        # the switch is live: the frame without it differs
        gp0, p0 = _frame_params(pkg, depth, mat, flags, 0.05)
        orc0 = ob.OracleRender(A, sc.desc, size, size)
        orc0.gbuffer(cam, gp0)
        orc0.bdpt(cam, p0, flags=oflags)
        assert not (np.array_equal(orc0.image(), orc.image()) and np.array_equal(orc0.splat, orc.splat)), name
        orc0.close()
        R = hi.Renderer(hi.Scene(sc.desc), cam, p, size, size, area=tab)
        assert R.nl == 2
        img = np.zeros((size, size, 4))
        spl = np.zeros((size * size, 4))
        for y in range(size):
            for x in range(size):
                i = y * size + x
                with np.errstate(all="ignore"):
                    o, ss = R.pixel(x, y, orc.chan["worldPosition"][i], orc.chan["worldNormal"][i], orc.chan["materialDiffuse"][i],
                                    orc.chan["materialSpecRough"][i], orc.chan["emissive"][i], **kw)
                img[y, x] = o
                for tx, ty, c in ss:
                    spl[ty * size + tx, :3] += c
                    spl[ty * size + tx, 3] += 1
        if name == "splat":
            same = spl[:, 3] == splat[:, 3]
            assert same.mean() > 0.95, same.mean()
            err = np.abs(spl[same, :3] - splat[same, :3]).max(axis=1)
            assert (err < 2e-5).mean() > 0.97, (err < 2e-5).mean()
            assert splat[:, 3].sum() > size * size / 4
        else:
            err = np.abs(img[..., :3] - own[..., :3]).max(axis=-1)
            ok = (err < 2e-5) & (img[..., 3] == own[..., 3])
            assert ok.mean() > 0.95, (name, ok.mean())
            assert (own[..., :3].sum(axis=-1) > 1e-5).mean() > 0.2, name
        orc.close()
