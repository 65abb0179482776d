"""The oracle's BDPT frame (oracle/bdpt_oracle.cpp) against the float64 reading of the ray-generation shader
(tests/hlsl_integrator_numpy.py) on the edge-case scenes of tests/edge_scenes.py, stage by stage as
test_integrator_matches_float64_reading_of_the_raygen_shader does on the Cornell box: NEE only, light-tracing splats only,
connections only (with ORACLE_CONNECT_ALL_VISIBLE; for `enclosed` and `open`, whose connection rays do not end on a tie, also
traced).  The own-pixel image is compared before the splat fold-in, the splat buffer per target pixel.  What the shader leaves
to the driver — which triangle a ray hits — comes from the oracle's own scan through hlsl_integrator_numpy.Scene(tracer=...),
so a comparison is about the integrator.

Classes first: the alpha word (the term count), the splat count of every target pixel and the NaN class of every channel must
be equal; then the values within bound_of(MEASURED[...]).  A pixel is left out only where the reading's own decision quantity
lies within a margin of a discontinuity (Renderer.risky), at most CAP of a case's pixels.  No GPU.
`python tests/test_edge_scenes_cpu.py` prints the tables edge_scenes.py records."""
import ctypes as C

import numpy as np
import pytest

import edge_scenes as es
import hlsl_integrator_numpy as hi

CASES = es.cases()
IDS = [c.id for c in CASES]
CPU_STAGES = (("nee", es.NO_SPLAT | es.NO_CONNECT, dict(splat=False, connect=False), False),
              ("splat", es.NO_NEE | es.NO_CONNECT, dict(nee=False, connect=False), False),
              ("connect", es.NO_NEE | es.NO_SPLAT, dict(nee=False, splat=False, connect_all_visible=True), True),
              ("connect_traced", es.NO_NEE | es.NO_SPLAT, dict(nee=False, splat=False), False))
TRACED = ("enclosed", "open")  # families whose connection rays end in free space or behind a wall, never on a tie
ORDINARY_BOUND = 2e-5          # the Cornell cross-check's


def key_of(case, stage):
    return f"{case.family}/{stage}"


def tie_case(case):
    """a light or the camera lies ON a surface: every next-event or light-tracing shadow ray ends on that surface, a last-bit
    decision that the GPU tests hold bit for bit; here both sides take such rays as unoccluded (ORACLE_TERMS_ALL_VISIBLE)"""
    return case.family == "light_on_surface" or (case.family == "camera" and case.variant in ("on_wall", "close")) or \
        (case.family == "mis" and case.variant.startswith("light_on_surface"))


def values_compared(case, stage):
    """False where only classes are held: class-only cases, and the connections of a scene with a 1e30 light — a pair of
    vertices in one plane has G = 0 exactly in fp32 and 1e-19 from float64 positions, times 1e30 that is past the clamp"""
    return not case.class_only and not (case.family == "intensity" and "big" in case.variant and stage.startswith("connect"))


class Tally:
    def __init__(self):
        self.worst, self.left_out, self.pixels, self.bad, self.nan_terms, self.nonfinite = 0.0, 0, 0, [], 0, 0


def _tracer(lib, osc, flags):
    ray, prim, tuv = np.zeros(8, np.float32), np.zeros(1, np.int32), np.zeros(3, np.float32)

    def trace(o, d, tmin, tmax):
        ray[0:3], ray[3:6], ray[6], ray[7] = o, d, tmin, tmax
        lib.oracle_trace(osc, ray.ctypes.data, 1, 0, flags, prim.ctypes.data, tuv.ctypes.data)
        return None if prim[0] < 0 else (int(prim[0]), float(tuv[0]), float(tuv[1]), float(tuv[2]))
    return trace


def compare(pkg, ob, case, stage, sem=hi.D3D):
    """one case, one stage of CPU_STAGES -> Tally"""
    name, flags, kw, all_visible = next(s for s in CPU_STAGES if s[0] == stage)
    A = pkg.abi
    lib = ob.load_oracle(A)
    oflags = ob.ORACLE_BRUTE_FORCE | (ob.ORACLE_CONNECT_ALL_VISIBLE if all_visible else 0) | \
        (ob.ORACLE_TERMS_ALL_VISIBLE if tie_case(case) else 0)
    kw = dict(kw, terms_all_visible=tie_case(case))
    r = es.oracle_case(pkg, ob, case, stages=((name, flags),), oflags=oflags)[0, name]
    sc = case.scene(A)
    cam = sc.camera(case.W / case.H)
    osc = lib.oracle_scene_create(C.byref(sc.desc))
    _, p = es.frame_params(pkg, case, 0, flags)
    mis = "power" if case.flags & es.MIS_POWER else "linear" if case.flags & es.MIS_LINEAR else None
    R = hi.Renderer(hi.Scene(sc.desc, tracer=_tracer(lib, osc, ob.ORACLE_BRUTE_FORCE)), cam, p, case.W, case.H,
                    specular_from_lobe=bool(case.flags & es.FROM_LOBE), mis=mis,
                    env_color=es.ENV_COLOR if case.flags & es.ENV_ON_MISS else None, sem=sem, margins=True)
    n = case.W * case.H
    img, spl, risky = np.zeros((n, 4)), np.zeros((n, 4)), np.zeros(n, bool)
    tainted = np.zeros(n, bool)  # splat targets a risky source pixel reaches in the reading
    ch = r.chan
    with np.errstate(all="ignore"):
        for i in range(n):
            o, ss = R.pixel(i % case.W, i // case.W, ch["worldPosition"][i], ch["worldNormal"][i], ch["materialDiffuse"][i],
                            ch["materialSpecRough"][i], ch["emissive"][i], **kw)
            img[i] = o
            risky[i] = bool(R.risky)
            for tx, ty, c in ss:
                spl[ty * case.W + tx, :3] += c
                spl[ty * case.W + tx, 3] += 1
                tainted[ty * case.W + tx] |= risky[i]
    lib.oracle_scene_destroy(osc)
    t = Tally()
    t.pixels, t.nan_terms = n, R.nan_terms
    own = r.own.astype(np.float64)
    splat = r.splat.astype(np.float64)
    splat[:, :3] /= 2.0 ** 32
    label = f"{case.id} {stage}"
    # ---- classes: alpha words, splat counts, NaN class
    keep = ~risky
    if not np.array_equal(own[keep, 3], img[keep, 3]):
        t.bad.append(f"{label}: alpha words differ at {np.nonzero(keep & (own[:, 3] != img[:, 3]))[0][:6].tolist()}")
    if not np.array_equal(np.isnan(own[keep, :3]), np.isnan(img[keep, :3])):
        t.bad.append(f"{label}: NaN class of the own-pixel image differs")
    count_off = splat[:, 3] != spl[:, 3]
    if count_off.any() and not risky.any():
        t.bad.append(f"{label}: splat counts differ at {np.nonzero(count_off)[0][:6].tolist()}")
    keep_t = ~(tainted | count_off)
    t.left_out = int(risky.sum()) + int((~keep_t & ~risky).sum() if name == "splat" else 0)
    t.nonfinite = int((~np.isfinite(own[:, :3])).sum())
    # ---- values
    if values_compared(case, stage):
        m = keep[:, None] & np.isfinite(own[:, :3]) & np.isfinite(img[:, :3])
        if m.any():
            t.worst = float(np.abs(own[:, :3] - img[:, :3])[m].max())
        if name == "splat" and keep_t.any():
            t.worst = max(t.worst, float(np.abs(splat[keep_t, :3] - spl[keep_t, :3]).max()))
    return t


_cache = {}


def tally_of(pkg, ob, case, stage):
    k = (case.id, stage)
    if k not in _cache:
        _cache[k] = compare(pkg, ob, case, stage)
    return _cache[k]


def stages_of(case):
    out = ["nee", "splat"]
    if case.depth >= 2:
        out.append("connect")
        if case.family in TRACED:
            out.append("connect_traced")
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_family_control_holds_on_the_oracle(pkg, ob, case):
    ok, seen = es.control_of(pkg, ob, case)
    assert ok, (case.id, seen)
    assert case.scene(pkg.abi).I.shape[0] <= 64


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_matches_float64_reading(pkg, ob, case):
    left = 0
    for stage in stages_of(case):
        t = tally_of(pkg, ob, case, stage)
        assert not t.bad, t.bad
        left = max(left, t.left_out)
        if values_compared(case, stage):
            bound = es.bound_of(es.MEASURED[key_of(case, stage)])
            assert t.worst <= bound, (case.id, stage, t.worst, bound)
            if case.family == "ordinary":
                assert t.worst <= ORDINARY_BOUND, (case.id, stage, t.worst)
    assert left <= es.LEFT_OUT.get(case.id, 0), (case.id, left)
    assert es.LEFT_OUT.get(case.id, 0) <= es.CAP * case.W * case.H, case.id


def test_intensity_reaches_nan_terms_before_the_clamp(pkg, ob):
    """the control of `intensity` on the reading's side: terms that are NaN before clampVec do occur, in every stage"""
    for stage in ("nee", "splat", "connect"):
        seen = sum(tally_of(pkg, ob, c, stage).nan_terms for c in CASES if c.family == "intensity" and (c.W, c.H) == (13, 5))
        assert seen > 0, stage


def test_oracle_refuses_a_clamp_upper_outside_the_fixed_point_range(pkg, ob):
    """include/bdpt.h, bdpt_params: NaN and negative bounds are BDPT_E_INVALID; above BDPT_MAX_CLAMP_UPPER_SPLAT a frame with
    the light-tracing stage is BDPT_E_LIMIT, one without it is taken (+inf included)"""
    A = pkg.abi
    lib = ob.load_oracle(A)
    case = es.Case("intensity", "inf_nan_0", 7, 5, 3, 1)
    sc = case.scene(A)
    cam = sc.camera(case.W / case.H)
    orc = ob.OracleRender(A, sc.desc, case.W, case.H)
    gp, p = es.frame_params(pkg, case, 0)
    orc.gbuffer(cam, gp)
    above = float(np.nextafter(np.float32(es.CLAMP_LIMIT), np.float32(np.inf)))

    def rc(clamp, flags):
        p.clampUpper, p.flags = clamp, flags
        return lib.oracle_bdpt(orc.scene, C.byref(cam), C.byref(p), C.byref(orc.frame), 0, 1, None)
    for clamp in (float("nan"), -1.0, -0.5, -float("inf")):
        assert rc(clamp, 0) == -1 and rc(clamp, es.NO_SPLAT) == -1, clamp
    for clamp in (above, es.FLT_MAX, float("inf")):
        assert rc(clamp, 0) == -5 and rc(clamp, es.NO_SPLAT) == 0, clamp
    for clamp in (0.0, 0.9, 1.0, es.CLAMP_LIMIT):
        assert rc(clamp, 0) == 0, clamp
    orc.close()


# ---- positive controls: the reading with one rule switched off must visibly miss a named case ------------------------------
def _case(cid):
    return next(c for c in CASES if c.id == cid)


def _misses(pkg, ob, cid, stage, sem):
    case = _case(cid)
    good = tally_of(pkg, ob, case, stage)
    assert not good.bad and good.worst <= es.bound_of(es.MEASURED[key_of(case, stage)]), "the unpatched reading must pass"
    t = compare(pkg, ob, case, stage, sem)
    return bool(t.bad) or t.worst > es.bound_of(es.MEASURED[key_of(case, stage)])


def test_reading_without_the_per_write_saturate_misses(pkg, ob):
    """BDPTMain.rt.hlsl:230: every connection write saturates; summed first, alpha counts the visible pairs"""
    assert _misses(pkg, ob, "ordinary 13x5 d3 m1", "connect", hi.Semantics(saturate_per_write=False))


def test_reading_with_a_nan_keeping_clamp_on_splats_misses(pkg, ob):
    """MaterialUtils.hlsli:15-18 under D3D's min / max: a NaN channel becomes +0 and the other two survive; with an IEEE clamp
    colorsNan (BDPTMain.rt.hlsl:197) fires and zeroes all three"""
    assert _misses(pkg, ob, "intensity/neg_nan_big 13x5 d3 m1", "splat", hi.Semantics(d3d_clamp=False))


def test_reading_that_skips_zero_valued_pairs_misses(pkg, ob):
    """BDPTMain.rt.hlsl:223-230: a visible pair whose contribution is zero still saturates the pixel and counts in alpha"""
    assert _misses(pkg, ob, "black 13x5 d3 m0", "connect", hi.Semantics(zero_pairs_write=False))


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as ge
    import oracle_binding
    package = ge.load_package()
    oracle_binding.load_oracle(package.abi)
    worst, left, bad = {}, {}, []
    for cs in CASES:
        for st in stages_of(cs):
            ty = tally_of(package, oracle_binding, cs, st)
            bad += ty.bad
            if values_compared(cs, st):
                worst[key_of(cs, st)] = max(worst.get(key_of(cs, st), 0.0), ty.worst)
            if ty.left_out:
                left[cs.id] = max(left.get(cs.id, 0), ty.left_out)
    print("MEASURED = {")
    for k, v in worst.items():
        print(f'    "{k}": {v:.1e},')
    print("}\nLEFT_OUT = {")
    for k, v in left.items():
        c = _case(k)
        print(f'    "{k}": {v},  # of {c.W * c.H}{"  OVER THE CAP" if v > es.CAP * c.W * c.H else ""}')
    print("}")
    for line in bad[:40]:
        print("#", line)
