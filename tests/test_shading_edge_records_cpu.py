"""The CPU oracle against the float64 readings of the shaders (tests/hlsl_reference_math.py,
tests/hlsl_light_connect_math.py) on the edge-case records of tests/edge_records.py, family by family: oracle_bsdf,
oracle_light_nee, oracle_connect_vertices and oracle_connect_camera.  No GPU: what the kernels make of the same records
is tests/test_gpu_shading_edge_records.py, bit for bit against this oracle.

Two classes of families:
  well-conditioned   the project's bounds (relative 5e-4 over a floor of 1e-4, directions within 1e-4), pixels and light
                     indices equal, the finite / non-finite pattern of every output word equal; at most 1 % of a family
                     left out by the margin rule
  ill-conditioned    the family sits on a comparison's boundary, where the two precisions may fall on different sides or
                     where a 0 / 0 waits: no magnitude is compared; the branch taken and the zero / finite / non-finite
                     class of every output word must agree on the rows the margin rule keeps, and the family must reach
                     its edge
The margin rule: a row is left out when a comparison it met lies within 1e-6 of its boundary in the float64 reading.
In the families of EXACT a margin of exactly 0 stays in: their records are fp32 numbers built so that the compared
quantity (a dot product with a zero in every term, or of two equal products) is exact in both precisions; both readings
then stand on the boundary itself and must take the same side.

`python tests/test_shading_edge_records_cpu.py` prints the table kept in the header of tests/edge_records.py.
"""
import numpy as np
import pytest

import edge_records as er
import hlsl_light_connect_math as lc
import hlsl_reference_math as hm

F = er.F
REL, FLOOR, DIR, MARGIN, CAP = 5e-4, 1e-4, 1e-4, 1e-6, 0.01
MIN_T = 1e-4


def _relerr(a, b):
    """per row: max over columns of |a - b| / (floor + |b|) where both are finite (the pattern is compared apart)"""
    a, b = np.asarray(a, np.float64).reshape(len(a), -1), np.asarray(b, np.float64).reshape(len(b), -1)
    with np.errstate(all="ignore"):
        e = np.abs(a - b) / (FLOOR + np.abs(b))
    return np.where(np.isfinite(a) & np.isfinite(b), e, 0.0).max(axis=1)


def _abserr(a, b):
    a, b = np.asarray(a, np.float64).reshape(len(a), -1), np.asarray(b, np.float64).reshape(len(b), -1)
    with np.errstate(all="ignore"):
        e = np.abs(a - b)
    return np.where(np.isfinite(a) & np.isfinite(b), e, 0.0).max(axis=1)


def _as32(x):
    with np.errstate(all="ignore"):
        return np.asarray(x, np.float64).astype(F)


def _cls(x):
    """0 zero, 1 finite and not zero, 2 not finite — of the value as an fp32 number"""
    x = _as32(x)
    return np.where(~np.isfinite(x), 2, np.where(x == 0, 0, 1))


EXACT = ("v_tangent", "l_tangent", "nl_zero", "tangent_planes")


def _left_out(margins, exact=False):
    """rows with a margin below MARGIN (NaN stays in; so does 0 in an EXACT family)"""
    m = np.asarray(margins, np.float64)
    return (((m > 0) if exact else (m >= 0)) & (m < MARGIN)).any(axis=1)


class Result:
    """one family of one call: the oracle's words (`got`), the float64 reading's (`ref`), which columns are directions,
    which integers, and the margins"""

    def __init__(self, got, ref, margins, dir_cols=(), int_cols=(), exact=False):
        self.got, self.ref, self.left = np.asarray(got, np.float64), np.asarray(ref, np.float64), _left_out(margins, exact)
        self.margins = np.asarray(margins, np.float64)
        n_col = self.got.shape[1]
        self.dirs, self.ints = list(dir_cols), list(int_cols)
        self.vals = [c for c in range(n_col) if c not in self.dirs and c not in self.ints]

    def errors(self):
        k = ~self.left
        rel = _relerr(self.got[k][:, self.vals], self.ref[k][:, self.vals]) if k.any() else np.zeros(0)
        d = _abserr(self.got[k][:, self.dirs], self.ref[k][:, self.dirs]) if (k.any() and self.dirs) else np.zeros(1)
        return float(rel.max()) if len(rel) else 0.0, float(d.max())

    def assert_well(self, what, cap=CAP):
        k = ~self.left
        assert self.left.mean() <= cap, f"{what}: {int(self.left.sum())} of {len(self.left)} rows left out by the margin rule"
        g, r = self.got[k], self.ref[k]
        assert np.array_equal(np.isfinite(_as32(g)), np.isfinite(_as32(r))), f"{what}: finite / non-finite pattern differs in " \
            f"{int((np.isfinite(_as32(g)) != np.isfinite(_as32(r))).any(axis=1).sum())} rows"
        if self.ints:
            assert np.array_equal(g[:, self.ints], r[:, self.ints]), f"{what}: integer outputs differ"
        rel, d = self.errors()
        assert rel < REL and d < DIR, f"{what}: worst relative error {rel:.3g}, worst direction error {d:.3g}"

    def assert_class(self, what):
        k = ~self.left
        g, r = self.got[k], self.ref[k]
        bad = (_cls(g) != _cls(r)).any(axis=1)
        if self.ints:
            bad |= (g[:, self.ints] != r[:, self.ints]).any(axis=1)
        assert not bad.any(), f"{what}: branch or zero / finite / non-finite class differs in {int(bad.sum())} of {int(k.sum())} rows " \
            f"outside the margin, first {int(np.nonzero(k)[0][np.argmax(bad)])}"


# ---- BSDF -------------------------------------------------------------------------------------------------------------
BSDF_WELL = er.BSDF_FIRST_GROUP + ("spec_one", "ggx_d_clamp", "ndoth_one", "luminance_clamp", "nonfinite_colour")
BSDF_ILL = ("rough_to_zero", "v_tangent", "l_tangent", "lobe_tie", "draw_edges")
_bsdf_cache = {}
_bsdf_fam = {}


def _bsdf(pkg, ob, name, mat):
    """columns: 0-2 weight, 3-5 L, 6 pdf, 7 the isSpecular flag, 8-10 f"""
    if (name, mat) in _bsdf_cache:
        return _bsdf_cache[(name, mat)]
    if name not in _bsdf_fam:
        _bsdf_fam[name] = er.bsdf_records(name)
    recs = _bsdf_fam[name]
    out = np.zeros((recs.n, 16), F)
    ob.load_oracle(pkg.abi).oracle_bsdf(recs.rec.ctypes.data, recs.n, mat, out.ctypes.data)
    ref, margins = np.zeros((recs.n, 11)), np.zeros((recs.n, 5))
    with np.errstate(all="ignore"):
        for i in range(recs.n):
            r = recs.rec[i, :17].astype(np.float64)
            n, v, l, dif, spec, rough = r[0:3], r[3:6], r[6:9], r[9:12], r[12:15], r[15]
            w, L, pdf, lobe, _ = hm.sample_brdf(mat & 1, int(recs.seeds[i]), n, v, dif, spec, rough)
            f = hm.eval_brdf(mat & 1, v, l, n, dif, spec, rough, recs.rec[i, 16] != 0)
            ref[i, 0:3], ref[i, 3:6], ref[i, 6], ref[i, 8:11] = w, L, pdf, f
            ref[i, 7] = 1.0 if (mat == 2 and lobe) else 0.0  # never written by sampleGGXBRDF: false, or the lobe with the flag
            m = hm.brdf_margins(mat & 1, int(recs.seeds[i]), n, v, l, dif, spec, rough, L)
            margins[i] = (m["lobe"], m["ndotl_sample"], m["ndotl_eval"], m["ndotv"], m["fp32_range"])
    res = Result(out[:, :11], ref, margins, dir_cols=(3, 4, 5), int_cols=(7,), exact=name in EXACT)
    res.recs = recs
    _bsdf_cache[(name, mat)] = res
    return res


@pytest.mark.parametrize("mat", [0, 1, 2])
@pytest.mark.parametrize("name", BSDF_WELL)
def test_bsdf_well_conditioned_families(pkg, ob, name, mat):
    """oracle_bsdf within the existing bounds of the float64 reading.  The families the issue names leave out no row."""
    res = _bsdf(pkg, ob, name, mat)
    res.assert_well(f"bsdf {name} mat {mat}", cap=0.0 if name in er.BSDF_FIRST_GROUP else CAP)


@pytest.mark.parametrize("mat", [0, 1, 2])
@pytest.mark.parametrize("name", BSDF_ILL)
def test_bsdf_ill_conditioned_families(pkg, ob, name, mat):
    """rough_to_zero: D = a2 / max(0.001, d^2 pi) with d = 1 - N.H^2 (1 - a2) cancels to the last bit as a2 -> 0, and below
    roughness 1e-19 fp32's a2 underflows where float64's does not (0 / 0 against a finite ratio): rows whose a2 or a2 / 2 is
    below FLT_MIN are inside that margin.  v_tangent, l_tangent: N.V or N.L is exactly 0: the specular term is 0 / 0 and the
    cosine test stands on its boundary.  lobe_tie: the first draw is within one fp32 step of probDiffuse, whose fp32 value is
    up to half a step off the float64 one.  draw_edges: a draw of 1 - 2^-24 makes (a2 - 1) r0 + 1 cancel to a few bits."""
    _bsdf(pkg, ob, name, mat).assert_class(f"bsdf {name} mat {mat}")


def test_bsdf_families_reach_their_edges(pkg, ob):
    fam = {k: er.bsdf_records(k) for k in ("rough_to_zero", "v_tangent", "l_tangent", "lobe_tie", "draw_edges", "luminance_clamp",
                                             "ggx_d_clamp", "ndoth_one", "first_draw_zero", "axis_normals", "nonfinite_colour")}
    out = {k: _bsdf(pkg, ob, k, 2).got for k in fam}
    r = fam["rough_to_zero"].rec
    assert (r[:, 15] == 0).sum() > 50 and ((r[:, 15] > 0) & (r[:, 15] * r[:, 15] == 0)).sum() > 20  # roughness 0, and a square that underflows
    assert np.isnan(out["rough_to_zero"][:, 0:3]).any() and np.isfinite(out["rough_to_zero"][:, 0:3]).all(axis=1).any()
    assert (er.dot3(fam["v_tangent"].rec[:, 0:3], fam["v_tangent"].rec[:, 3:6]) == 0).all() and np.isnan(out["v_tangent"]).any()
    assert (er.dot3(fam["l_tangent"].rec[:, 0:3], fam["l_tangent"].rec[:, 6:9]) == 0).all() and (out["l_tangent"][:, 8:11] == 0).all()
    t = fam["lobe_tie"]
    _, draw = er.lcg(t.seeds)
    pd = er._prob_diffuse32(t.rec[:, 9:12], t.rec[:, 12:15])
    gap = (pd.astype(np.float64) - draw) * 2 ** 24
    assert (gap == 0).sum() > 20 and ((gap > 0) & (gap <= 1)).sum() > 20 and ((gap < 0) & (gap >= -1)).sum() > 20
    assert 0 < (out["lobe_tie"][:, 7] == 1).sum() < t.n  # both lobes
    s = fam["draw_edges"].seeds
    draws = []
    for _ in range(3):
        s, r = er.lcg(s)
        draws.append(r)
    assert all((d == 0).sum() > 20 and (d == F(1.0) - F(2.0 ** -24)).sum() > 20 for d in draws)
    assert (er.lcg(fam["first_draw_zero"].seeds)[1] == 0).all()
    w = np.array([0.2126, 0.7152, 0.0722], F)
    lum = er.dot3(fam["luminance_clamp"].rec[:, 9:12], w[None])
    assert (lum < F(0.01)).sum() > 20 and (lum > F(0.01)).sum() > 20
    g = fam["ggx_d_clamp"].rec
    h = er.normalize3((g[:, 6:9] + g[:, 3:6]).astype(F))
    a2 = g[:, 15] * g[:, 15]
    ndh = er.dot3(g[:, 0:3], h)
    d = (ndh * a2 - ndh) * ndh + F(1)
    assert ((d * d * er.PI32) < F(0.001)).sum() > 20 and ((d * d * er.PI32) > F(0.001)).sum() > 20
    g = fam["ndoth_one"].rec
    assert (er.dot3(g[:, 0:3], er.normalize3((g[:, 6:9] + g[:, 3:6]).astype(F))) == 1).sum() > 100
    assert np.signbit(fam["axis_normals"].rec[:, 0:3]).any() and (fam["axis_normals"].rec[:, 0:3] == 0).sum() == 2 * fam["axis_normals"].n
    assert np.isnan(out["nonfinite_colour"]).any() and np.isinf(fam["nonfinite_colour"].rec[:, 9:15]).any()


# ---- lights -----------------------------------------------------------------------------------------------------------
_light_cache = {}


def _light_cases():
    if "cases" not in _light_cache:
        _light_cache["cases"] = {c.name: c for c in er.light_cases()}
    return _light_cache["cases"]


LIGHT_FAMILIES = [(c.name, f) for c in er.light_cases() for f in c.names]


def _light(pkg, ob, case_name, mat):
    """columns: 0-2 L, 3 distance, 4-6 value, 7 light, 8 status"""
    if (case_name, mat) in _light_cache:
        return _light_cache[(case_name, mat)]
    c = _light_cases()[case_name]
    got, after = ob.light_nee(pkg.abi, er.make_lights(pkg.abi, c.lights), c.surf, c.seeds, mat, MIN_T)
    assert np.array_equal(after, er.lcg(c.seeds)[0])
    assert np.array_equal(got[:, 0:3].view(np.uint32)[c.surf.view(np.int32)[:, 23] >= 0], c.surf[:, 0:3].view(np.uint32)[c.surf.view(np.int32)[:, 23] >= 0])
    word = got.view(np.uint32)[:, 11]
    assert ((word & 0xFFFF) < len(c.lights)).all()  # the index every later GPU run will use: in range
    o = np.concatenate([got[:, 4:11].astype(np.float64), (word & 0xFFFF)[:, None], (word >> 16)[:, None]], axis=1)
    ref, margins = np.zeros((c.n, 9)), np.ones((c.n, 7))
    with np.errstate(all="ignore"):
        for i in range(c.n):
            s = c.surf[i].astype(np.float64)
            if c.surf.view(np.int32)[i, 23] < 0:
                ref[i, 7] = 0  # an all-zero sample
                continue
            lr = float(c.surf[i, 7])
            idx, L, dist, val, m = lc.light_nee(c.lights, int(c.seeds[i]), mat, s[0:3], s[4:7], s[8:11], s[12:15], s[16:19],
                                                float(F(lr) * F(lr)))
            ref[i, 0:3], ref[i, 3], ref[i, 4:7], ref[i, 7] = L, dist, val, idx
            ref[i, 8] = 0.0 if (_as32(val) == 0).all() else 1.0
            margins[i] = (m["dist2"], m["cone"], m["ndotl"], m["ndotv"], m["select"], m["fp32_range"], m["acos_domain"])
    res = Result(o, ref, margins, dir_cols=(0, 1, 2), int_cols=(7,))
    res.case = c
    _light_cache[(case_name, mat)] = res
    return res


def _family(res, batch, fam):
    k = batch.of(fam)
    return Result(res.got[k], res.ref[k], res.margins[k], res.dirs, res.ints, exact=fam in EXACT)


@pytest.mark.parametrize("mat", [0, 1])
@pytest.mark.parametrize("case_name,fam", LIGHT_FAMILIES)
def test_light_families(pkg, ob, case_name, fam, mat):
    """oracle_light_nee against the float64 reading of getLightData and the two *Direct functions.  Ill-conditioned:
    dist2_threshold (distance^2 within a few steps of the 1e-5 switch: normalize or zero), nl_zero (N.L exactly 0: the GGX
    masking term is 0 / 0), cone_edge (cosTheta equal to cosOpeningAngle or one step off: falloff or none),
    opening_and_dir (openingAngle 0 with points on the axis, where cosTheta is 1 or a rounding below it against
    cosOpeningAngle 1; a dirW three times unit length, where cosTheta passes 1 and the shader's acos leaves its domain:
    the build's definition, acos of the clamped argument, is asserted by test_light_families_reach_their_edges, not
    arbitrated by the float64 reading, which keeps HLSL's NaN and leaves those rows out)."""
    res = _light(pkg, ob, case_name, mat)
    sub = _family(res, res.case, fam)
    if fam in res.case.ill:
        sub.assert_class(f"light {case_name}/{fam} mat {mat}")
    else:
        sub.assert_well(f"light {case_name}/{fam} mat {mat}")


def test_light_families_reach_their_edges(pkg, ob):
    cases = _light_cases()
    c = cases["one_point"]
    lp = np.array(c.lights[0]["posW"], F)
    v = (lp[None] - c.surf[:, 0:3]).astype(F)
    d2 = er.dot3(v, v)
    k = c.of("dist2_threshold")
    assert (d2[k] > F(1e-5)).sum() > 20 and ((d2[k] <= F(1e-5)) & (d2[k] > 0)).sum() > 20 and (d2[k] == 0).sum() > 20
    assert np.isinf(d2[c.of("dist2_overflow")]).all()
    got = _light(pkg, ob, "one_point", 0).got
    assert (er.dot3(c.surf[:, 4:7], er.normalize3(er.normalize3(v)))[c.of("nl_zero")] == 0).all()
    assert (got[c.of("back_facing")][:, 4:7] <= 0).all() or np.isnan(got[c.of("back_facing")][:, 4:7]).any()
    assert np.isnan(got[c.of("v_is_minus_l")][:, 4:7]).all()  # normalize(V + L) = normalize(0)
    assert (got[c.of("miss")] == 0).all()
    t = cases["one_point_tiny"]
    v = (np.array(t.lights[0]["posW"], F)[None] - t.surf[:, 0:3]).astype(F)
    assert (er.dot3(v, v) == 0).all() and (v != 0).any(axis=1).all()
    e = cases["cone_edge"]
    k = e.of("cone_edge")
    lsl = er.normalize3((np.array(e.lights[0]["posW"], F)[None] - e.surf[:, 0:3]).astype(F))
    cos_open = np.array([l["cosOpeningAngle"] for l in e.lights], F)[e.which]
    assert ((lsl[:, 2] == cos_open) & k).sum() > 20 and ((lsl[:, 2] < cos_open) & k).sum() > 20 and ((lsl[:, 2] > cos_open) & k).sum() > 20
    ge = _light(pkg, ob, "cone_edge", 1).got
    assert (ge[k & (lsl[:, 2] < cos_open)][:, 4:7] == 0).all() and (ge[k & (lsl[:, 2] == cos_open)][:, 4:7] != 0).any()
    for count in (3, 4):
        s = cases[f"selection_{count}"]
        _, r = er.lcg(s.seeds)
        x = r * F(count)
        assert (x == np.floor(x)).sum() > 20 and set(s.which) == set(range(count)) and (r == F(1.0) - F(2.0 ** -24)).any()
        assert np.array_equal(_light(pkg, ob, f"selection_{count}", 1).got[:, 7], s.which)
    # opening_and_dir: light 0 has openingAngle 0 (cosOpeningAngle 1), 1 is a point light, 2 a spot with a zero dirW, 3 one
    # with dirW = (0, 0, -3)
    o = cases["opening_and_dir"]
    go = _light(pkg, ob, "opening_and_dir", 1).got
    lsl = er.normalize3((np.array([l["posW"] for l in o.lights], F)[o.which] - o.surf[:, 0:3]).astype(F))
    cos_t = -er.dot3(lsl, np.array([l["dirW"] for l in o.lights], F)[o.which])
    lit = (go[:, 4:7] != 0).any(axis=1)
    axis = (o.which == 0) & (lsl[:, 0] == 0) & (lsl[:, 1] == 0)
    assert o.lights[0]["cosOpeningAngle"] == 1.0 and axis.sum() > 20
    facing = er.dot3(o.surf[:, 4:7], er.normalize3(lsl)) > 0
    # lit exactly where cosTheta == cosOpeningAngle == 1 (and the surface faces the light)
    assert np.array_equal(lit[o.which == 0], ((cos_t == 1) & facing)[o.which == 0])
    assert 0 < (axis & lit).sum() < axis.sum()  # normalize() leaves some axis rows one step below 1: unlit
    assert np.array_equal(lit[o.which == 1], facing[o.which == 1])
    assert (cos_t[o.which == 2] == 0).all() and not lit[o.which == 2].any()  # zero dirW: cosTheta 0 < cos(0.6) everywhere
    past = (o.which == 3) & (cos_t > 1)
    # the build's acos clamps: past cosTheta = 1 the penumbra term is saturate((0.6 - 0 - 0.2) / 0.2) = 1, the light is lit
    assert past.sum() > 20 and np.array_equal(lit[past], facing[past]) and lit[past].any() and np.isfinite(go[past][:, 4:7]).all()
    gi = _light(pkg, ob, "intensity", 1).got
    assert np.isinf(gi[:, 4:7]).any() and (gi[:, 4:7] < 0).any() and (gi[:, 4:7] > 1e20).any()


# ---- vertex connections -----------------------------------------------------------------------------------------------
_vertex_cache = {}
VERTEX_FAMILIES = list(er.vertex_families())


def _vertex_dict(rec, i, spec_flag, ggx):
    s = rec[i].astype(np.float64)
    lr = F(rec[i, 7])
    return dict(pos=s[0:3], N=s[4:7], V=s[8:11], dif=s[12:15], spec=s[16:19] if ggx else np.zeros(3), rough=float(lr * lr) if ggx else 0.0,
                is_spec=bool(spec_flag) and ggx)


def _vertex(pkg, ob, name, mat, with_prev):
    """columns: 0-2 dir, 3 tmax, 4-6 value, 7 status"""
    key = (name, mat, with_prev)
    if key in _vertex_cache:
        return _vertex_cache[key]
    v = er.vertex_records(name)
    got = ob.connect_vertices(pkg.abi, v.eye, v.light, mat, MIN_T, v.eye_prev if with_prev else None, v.light_prev if with_prev else None,
                              v.eye_spec, v.light_spec)
    assert np.array_equal(got[:, 0:3].view(np.uint32), v.eye[:, 0:3].view(np.uint32)) and (got[:, 3] == F(MIN_T)).all()
    o = np.concatenate([got[:, 4:11].astype(np.float64), got.view(np.uint32)[:, 11:12]], axis=1)
    ref, margins = np.zeros((v.n, 8)), np.ones((v.n, 5))
    with np.errstate(all="ignore"):
        for i in range(v.n):
            e, l = _vertex_dict(v.eye, i, v.eye_spec[i], mat == 0), _vertex_dict(v.light, i, v.light_spec[i], mat == 0)
            vec = l["pos"] - e["pos"]
            ref[i, 3] = np.linalg.norm(vec)
            ref[i, 0:3] = vec / np.float64(ref[i, 3])
            if v.eye.view(np.int32)[i, 23] < 0 or v.light.view(np.int32)[i, 23] < 0:
                continue
            wo_e = lc._norm(v.eye_prev[i, 0:3].astype(np.float64) - e["pos"]) if with_prev else e["V"]
            wo_l = lc._norm(v.light_prev[i, 0:3].astype(np.float64) - l["pos"]) if with_prev else l["V"]
            val, _, m = lc.connect_vertices(mat, e, l, wo_e, wo_l)
            ref[i, 4:7] = val
            ref[i, 7] = 0.0 if (_as32(val) == 0).all() else 1.0
            margins[i] = (m["ndotl_light"], m["ndotl_eye"], m["ndotv_light"], m["ndotv_eye"], m["fp32_range"])
    res = Result(o, ref, margins, dir_cols=(0, 1, 2), exact=name in EXACT)
    res.recs = v
    _vertex_cache[key] = res
    return res


@pytest.mark.parametrize("with_prev", [False, True])
@pytest.mark.parametrize("mat", [0, 1])
@pytest.mark.parametrize("name", VERTEX_FAMILIES)
def test_vertex_families(pkg, ob, name, mat, with_prev):
    """oracle_connect_vertices against the float64 reading of evalGWithoutV and the two BRDFs.  Ill-conditioned: coincident
    and one_step_apart (the connection direction is normalize(0) or one rounding of a difference), apart_1e-20 and
    apart_1e20 (length^2 under- or overflows in fp32 only), tangent_planes (both cosines exactly 0: G is 0 and the GGX terms
    0 / 0), connectdir_is_wol (woL is connectDir bit for bit, where L.H is 1 and the Fresnel term's (1 - L.H)^5 is 0, or
    its negation, where the cosine test cuts fsL to 0 or, with the normal turned away from the eye, the half vector is
    normalize(0): NaN for the specular lobe, dif / pi for the diffuse one), prev_is_vertex (an outgoing direction
    normalize(0): NaN where the vertex's specular flag is set, the diffuse lobe otherwise, whose cosine test a NaN passes), fsl_zero / fse_zero (the cosine test of a direction exactly opposite the normal's side)."""
    res = _vertex(pkg, ob, name, mat, with_prev)
    if name in er.VERTEX_ILL:
        res.assert_class(f"vertices {name} mat {mat} prev {with_prev}")
    else:
        res.assert_well(f"vertices {name} mat {mat} prev {with_prev}")


def test_vertex_families_reach_their_edges(pkg, ob):
    got = {k: _vertex(pkg, ob, k, 0, True).got for k in VERTEX_FAMILIES}
    assert (got["coincident"][:, 3] == 0).all() and np.isnan(got["coincident"][:, 0:3]).all()
    assert (got["one_step_apart"][:, 3] > 0).any()
    one = er.vertex_records("one_step_apart")
    moved = one.light[:, 0:3] != one.eye[:, 0:3]
    assert (moved.sum(axis=1) == 1).all() and np.array_equal(one.light[:, 0:3][moved], np.nextafter(one.eye[:, 0:3][moved], F(np.inf)))
    # connectdir_is_wol: the outgoing direction the hook uses is +-connectDir bit for bit, from V and from the predecessor
    c = er.vertex_records("connectdir_is_wol")
    k = np.arange(c.n) % 4
    cd = er.normalize3((c.eye[:, 0:3] - c.light[:, 0:3]).astype(F))
    sgn = np.where(k == 0, F(1), F(-1))[:, None]
    for wo_l in (c.light[:, 8:11], er.normalize3((c.light_prev[:, 0:3] - c.light[:, 0:3]).astype(F))):
        assert np.array_equal(wo_l.view(np.uint32), (sgn * cd).astype(F).view(np.uint32))
    for with_prev in (False, True):
        g = _vertex(pkg, ob, "connectdir_is_wol", 0, with_prev).got
        assert (np.isfinite(g[k == 0][:, 4:7]).all(axis=1) & (g[k == 0][:, 7] == 1)).sum() > 20
        assert (g[k == 1][:, 4:8] == 0).all()
        assert np.isnan(g[k == 2][:, 4:7]).all(axis=1).sum() > 20 and not np.isnan(g[k != 2][:, 4:7]).any()
        assert np.isfinite(g[k == 3][:, 4:7]).all() and (g[k == 3][:, 7] == 1).sum() > 20
    # prev_is_vertex: NaN only where the vertex whose predecessor coincides has its specular flag set
    p = er.vertex_records("prev_is_vertex")
    even = np.arange(p.n) % 2 == 0
    flagged = np.where(even, p.eye_spec, p.light_spec) != 0
    nan = np.isnan(got["prev_is_vertex"][:, 4:7]).any(axis=1)
    assert nan.sum() > 50 and not nan[~flagged].any() and (got["prev_is_vertex"][~flagged][:, 7] == 1).all()
    assert np.isfinite(got["prev_is_vertex"][~flagged][:, 4:7]).all()
    wo = er.normalize3((p.eye_prev[even, 0:3] - p.eye[even, 0:3]).astype(F))
    assert np.isnan(wo).all()
    lam = {k: _vertex(pkg, ob, k, 1, False).got for k in ("apart_1e-20", "apart_1e20", "apart_1e15", "tangent_planes")}
    assert np.isinf(lam["apart_1e-20"][:, 4:7]).any()      # invLengthAB^2 overflows
    assert np.isnan(lam["apart_1e20"][:, 0:3]).all() or np.isinf(lam["apart_1e20"][:, 3]).all()  # length^2 overflows
    assert np.isfinite(lam["apart_1e15"][:, 4:7]).all() and (lam["apart_1e15"][:, 4:7] < 1e-25).all()
    assert (lam["tangent_planes"][:, 4:7] == 0).all()
    assert (got["fsl_zero"][:, 4:8] == 0).all() and (got["fse_zero"][:, 4:8] == 0).all()
    m = er.vertex_records("miss")
    dead = (m.eye.view(np.int32)[:, 23] < 0) | (m.light.view(np.int32)[:, 23] < 0)
    assert 0 < dead.sum() < m.n and (got["miss"][dead][:, 4:8] == 0).all() and (got["miss"][~dead][:, 7] == 1).any()
    s = er.vertex_records("spec_flags")
    assert set(zip(s.eye_spec.tolist(), s.light_spec.tolist())) == {(0, 0), (0, 1), (1, 0), (1, 1)}


# ---- camera connections -----------------------------------------------------------------------------------------------
_camera_cache = {}
CAMERA_FAMILIES = ("ordinary", "edge_x", "edge_y", "corner", "tie_x", "tie_y", "camera_plane", "behind", "at_camera", "far_1e20",
                   "v_is_minus_dir", "miss")


def _camera(pkg, ob, frame, name, mat):
    """columns: 0-2 dir, 3 tmax, 4-6 f, 7 G, 8 pixel (-1: none), 9 the PIXEL bit, 10 the NONZERO bit"""
    key = (frame, name, mat)
    if key in _camera_cache:
        return _camera_cache[key]
    W, H, jit = er.FRAMES[frame]
    cam = er.origin_camera(pkg.abi)
    camt = er.camera_of(cam)
    if ("fam", frame) not in _camera_cache:
        _camera_cache[("fam", frame)] = er.camera_families(camt, W, H, jit)
    d = _camera_cache[("fam", frame)][name]
    rec = er.CameraRecords(d, np.zeros(len(d["light"]), np.int32), [name], W, H, jit)
    got = ob.connect_camera(pkg.abi, cam, W, H, jit, rec.light, mat, MIN_T, rec.light_spec)
    word = got.view(np.uint32)
    pix = word[:, 12].astype(np.int64)
    assert ((pix < W * H) | (pix == 0xFFFFFFFF)).all()  # the pixel every later GPU run hands to bdpt_splat_add: in range
    pix[pix == 0xFFFFFFFF] = -1
    o = np.concatenate([got[:, 4:12].astype(np.float64), pix[:, None], (word[:, 13:14] >> 1) & 1, word[:, 13:14] & 1], axis=1)
    cam64 = tuple(a.astype(np.float64) for a in camt)
    ref, margins = np.zeros((rec.n, 11)), np.ones((rec.n, 9))
    ref[:, 8] = -1
    with np.errstate(all="ignore"):
        for i in range(rec.n):
            if rec.light.view(np.int32)[i, 23] < 0:
                continue
            lv = _vertex_dict(rec.light, i, rec.light_spec[i], mat == 0)
            p, f, g, dr, dist, m = lc.connect_camera(mat, cam64, W, H, jit, lv)
            ref[i, 0:3], ref[i, 3], ref[i, 4:7], ref[i, 7] = dr, dist, f, g
            ref[i, 8], ref[i, 9] = (-1, 0) if p is None else (p, 1)
            ref[i, 10] = 1.0 if (p is not None and (_as32(f) != 0).any() and _as32(g) != 0) else 0.0
            margins[i] = [m.get(k, 1.0) for k in ("facing", "left", "right", "top", "bottom", "tie", "ndotl", "ndotv", "fp32_range")]
    res = Result(o, ref, margins, dir_cols=(0, 1, 2), int_cols=(8, 9))
    res.recs = rec
    _camera_cache[key] = res
    return res


@pytest.mark.parametrize("mat", [0, 1])
@pytest.mark.parametrize("name", CAMERA_FAMILIES)
@pytest.mark.parametrize("frame", range(len(er.FRAMES)))
def test_camera_families(pkg, ob, frame, name, mat):
    """oracle_connect_camera against the float64 reading of the splat's facing test, getLaunchIndexFromDirection, G and
    connectToCamera.  Ill-conditioned: edge_x / edge_y / corner (the target's coordinate on a frame edge's rounding boundary,
    or a step off), tie_x / tie_y (px W - jx = k + 0.5: rintf rounds to even, and a half step decides the pixel),
    camera_plane (dot(cameraN, dir) is 0 or a subnormal: facing or not, nx = +-inf), at_camera (distance 0: normalize(0)),
    far_1e20 (distance^2 overflows in fp32 only), v_is_minus_dir (the half vector is normalize(0) in fp32 and the
    normalised rounding of the direction in float64; N.V = 0 after its saturate makes the value 0 / 0 in both)."""
    res = _camera(pkg, ob, frame, name, mat)
    if name in er.CAMERA_ILL:
        res.assert_class(f"camera {name} frame {er.FRAMES[frame]} mat {mat}")
    else:
        res.assert_well(f"camera {name} frame {er.FRAMES[frame]} mat {mat}")


@pytest.mark.parametrize("frame", range(len(er.FRAMES)))
def test_camera_families_reach_their_edges(pkg, ob, frame):
    W, H, jit = er.FRAMES[frame]
    camt = er.camera_of(er.origin_camera(pkg.abi))
    res = {k: _camera(pkg, ob, frame, k, 1) for k in CAMERA_FAMILIES}
    t = {k: er.splat_target32(camt, res[k].recs.light[:, 0:3], W, H, jit) for k in CAMERA_FAMILIES}
    for name, axis in (("tie_x", 1), ("tie_y", 2)):
        g = t[name][axis]
        tie = g - np.floor(g) == 0.5
        assert (tie & (np.floor(g) % 2 == 0)).sum() > 10 and (tie & (np.floor(g) % 2 == 1)).sum() > 10, name
    _, gx, gy, fx, fy, inside, _ = t["corner"]
    pix = res["corner"].got[:, 8]
    assert (fx == W - 1).any() and (fx == W).any() and ((fx == 0) & np.signbit(fx)).any() and (fy == H - 1).any() and (fy == H).any()
    for x in (0, W - 1):
        for y in (0, H - 1):
            assert (pix == x + y * W).any(), (x, y)  # every corner pixel
    for g, size in ((gx, W), (t["edge_y"][2], H)):  # on a rounding boundary exactly, and within 1e-5 of both on either side
        assert ((g == F(-0.5)) | (g == F(size - 0.5))).sum() > 10
        for b in (-0.5, size - 0.5):
            assert ((g > b) & (g < b + 1e-5)).any() and ((g < b) & (g > b - 1e-5)).any(), (size, b)
    assert (res["edge_x"].got[:, 8] % W == W - 1).any() and (res["edge_y"].got[:, 8] // W == H - 1).any()
    facing, gx, _, _, _, _, d3 = t["camera_plane"]
    with np.errstate(all="ignore"):
        sub = (d3 != 0) & (np.abs(d3) < F(1.1754944e-38))
    assert (d3 == 0).sum() > 20 and sub.sum() > 20 and np.isinf(gx[facing]).any() and (res["camera_plane"].got[:, 8] == -1).all()
    assert (res["behind"].got[:, 8] == -1).all() and (res["behind"].got[:, 4:8] == 0).all()
    a = res["at_camera"].got
    assert (a[::2, 3] == 0).all() and np.isnan(a[::2, 0:3]).all() and (a[:, 8] == -1).all()
    assert np.isinf(res["far_1e20"].got[:, 3]).all()
    assert (res["miss"].got == np.array([0] * 8 + [-1, 0, 0])).all()
    ggx = _camera(pkg, ob, frame, "v_is_minus_dir", 0).got
    assert (np.isnan(ggx[:, 4:7]).all(axis=1) & (ggx[:, 8] >= 0)).sum() > 20  # a NaN f with a pixel


# ---- the pass's model: what the caller makes of a value ------------------------------------------------------------------
def _clamp_vec32(v, hi):
    """clampVec (MaterialUtils.hlsli:15-18) in fp32: clamp(x, 0, hi) with HLSL's rule that the other operand wins over NaN"""
    y = np.where(v > 0, v, F(0))
    return np.where(y < hi, y, hi).astype(F)


def _assert_pass_model(values, what):
    """clampVec((prevColor * value) / k, clampUpper) with positive and with zero throughputs and k = 2, 3: a NaN, a
    negative number or a zero of either sign comes out as +0 bit for bit; +inf, the one non-finite value the clamp does
    not drop, comes out as clampUpper."""
    values = np.ascontiguousarray(values, F)
    rng = np.random.default_rng(5)
    hi = F(0.9)
    for prev in (rng.uniform(0.05, 1.0, values.shape).astype(F), np.zeros(values.shape, F)):
        for k in (2, 3):
            with np.errstate(all="ignore"):
                term = (prev * values) / F(k)
                out = _clamp_vec32(term, hi)
            drop = np.isnan(term) | (term <= 0)
            assert (out[drop].view(np.uint32) == 0).all(), what
            assert (out[np.isposinf(term)] == hi).all() and np.isfinite(out).all() and (out >= 0).all() and (out <= hi).all(), what
            assert not np.isnan(out).any(), what
    bad = ~np.isfinite(values) | (values < 0)
    assert bad.any(), f"{what}: the families hold no non-finite or negative value"
    return int(bad.sum())


def test_pass_model_light_values(pkg, ob):
    vals = np.concatenate([_light(pkg, ob, c, mat).got[:, 4:7] for c in _light_cases() for mat in (0, 1)])
    _assert_pass_model(vals, "light values")


def test_pass_model_vertex_values(pkg, ob):
    vals = np.concatenate([_vertex(pkg, ob, k, mat, True).got[:, 4:7] for k in VERTEX_FAMILIES for mat in (0, 1)])
    _assert_pass_model(vals, "connection values")


def test_pass_model_camera_values(pkg, ob):
    """(prevColor * f) * G, the pass's order"""
    parts = []
    for k in CAMERA_FAMILIES:
        g = _camera(pkg, ob, 0, k, 0).got
        with np.errstate(all="ignore"):
            parts.append(_as32(g[:, 4:7]) * _as32(g[:, 7:8]))
    _assert_pass_model(np.concatenate(parts), "splat values")


def test_pass_model_bsdf_weights(pkg, ob):
    vals = np.concatenate([_bsdf(pkg, ob, k, 2).got[:, 0:3] for k in BSDF_WELL + BSDF_ILL])
    _assert_pass_model(vals, "sample weights")


# ---- the measured table -------------------------------------------------------------------------------------------------
def report(pkg, ob):
    rows = []
    for name in BSDF_WELL + BSDF_ILL:
        for mat in (0, 1, 2):
            r = _bsdf(pkg, ob, name, mat)
            rel, d = r.errors()
            rows.append((f"bsdf/{name}", mat, len(r.left), int(r.left.sum()), "class" if name in BSDF_ILL else f"rel {rel:.1e} dir {d:.1e}"))
    for case_name, fam in LIGHT_FAMILIES:
        for mat in (0, 1):
            res = _light(pkg, ob, case_name, mat)
            r = _family(res, res.case, fam)
            rel, d = r.errors()
            rows.append((f"light/{case_name}/{fam}", mat, len(r.left), int(r.left.sum()), "class" if fam in res.case.ill else f"rel {rel:.1e} dir {d:.1e}"))
    for name in VERTEX_FAMILIES:
        for mat in (0, 1):
            r = _vertex(pkg, ob, name, mat, True)
            rel, d = r.errors()
            rows.append((f"vertices/{name}", mat, len(r.left), int(r.left.sum()), "class" if name in er.VERTEX_ILL else f"rel {rel:.1e} dir {d:.1e}"))
    for name in CAMERA_FAMILIES:
        for mat in (0, 1):
            worst, left, n = (0.0, 0.0), 0, 0
            for frame in range(len(er.FRAMES)):
                r = _camera(pkg, ob, frame, name, mat)
                e = r.errors()
                worst, left, n = (max(worst[0], e[0]), max(worst[1], e[1])), left + int(r.left.sum()), n + len(r.left)
            rows.append((f"camera/{name}", mat, n, left, "class" if name in er.CAMERA_ILL else f"rel {worst[0]:.1e} dir {worst[1]:.1e}"))
    return rows


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as ge
    import oracle_binding
    _pkg = ge.load_package()
    oracle_binding.load_oracle(_pkg.abi)
    print(f"{'family':44s} mat  rows  left out  worst error against float64")
    for row in report(_pkg, oracle_binding):
        print(f"{row[0]:44s} {row[1]:3d} {row[2]:5d} {row[3]:9d}  {row[4]}")
