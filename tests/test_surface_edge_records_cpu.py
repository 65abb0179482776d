"""The oracle's hit shading and alpha test (oracle_shade_hits, oracle_alpha_test: loops over prepareShadingData and
alphaTestFails) against the float64 reading (tests/hlsl_textured_numpy.py), per family of tests/edge_surfaces.py.  No GPU.

Well-conditioned families: every field, within the bound edge_surfaces.BOUNDS derives from the measured deviations.
Ill-conditioned ones (edge_surfaces.ILL): the class only (pass / fail, normal flipped or not, finite / NaN), on the rows
outside a margin of 1e-6 in the reading's own decision quantity; the count of rows inside the margin is asserted and is at
most half the family.  Each family also asserts, with the fp32 restatement of the UV and fraction arithmetic, that it
reaches its edge.  `python tests/test_surface_edge_records_cpu.py` prints the measured table."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import edge_surfaces as es
from edge_surfaces import F, texel32

NMAP = 1  # BDPT_SHADE_NORMAL_MAP
INT_LIMIT = 2.0 ** 31


class World:
    """the scene, its oracle twin, the float64 reading and every family's records with both answers, made once"""

    def __init__(self, pkg, ob):
        from hlsl_textured_numpy import TexturedScene
        self.pkg, self.ob = pkg, ob
        self.sc = es.EdgeScene(pkg.abi)
        self.lib = ob.load_oracle(pkg.abi)
        self.osc = self.lib.oracle_scene_create(C.byref(self.sc.desc))
        self.reading = TexturedScene(self.sc.desc)
        self.fam = es.families(self.sc)
        self.rec = {k: es.SurfaceRecords(v, np.zeros(len(v["prim"]), np.int32), [k]) for k, v in self.fam.items()}
        self._cache = {}

    def oracle(self, name, flags=0):
        r = self.rec[name]
        return self.ob.shade_hits(self.pkg.abi, self.osc, r.rays, r.hits, flags)

    def read(self, name, flags=0):
        """(n, 24) float64 records of the reading, NaN rows where it cannot be evaluated (a UV that is not finite)"""
        key = (name, flags)
        if key not in self._cache:
            r, sc = self.rec[name], self.reading
            out = np.full((r.n, 24), np.nan)
            P = self.sc.P.astype(np.float64)[self.sc.I]
            for i in range(r.n):
                prim, u, v = int(r.prim[i]), float(r.uv[i, 0]), float(r.uv[i, 1])
                o = r.org[i].astype(np.float64)
                with np.errstate(all="ignore"):
                    pos = P[prim, 0] * (1.0 - u - v) + P[prim, 1] * u + P[prim, 2] * v
                try:
                    with np.errstate(all="ignore"):
                        s = sc.shade(prim, u, v, o, pos - o, 1.0, o, bool(flags & NMAP))
                except (ValueError, OverflowError):
                    continue
                with np.errstate(all="ignore"):
                    out[i, 0:3], out[i, 3], out[i, 4:7], out[i, 7] = pos, np.linalg.norm(pos - o), s["N"], s["linear_roughness"]
                out[i, 8:11], out[i, 11], out[i, 12:15], out[i, 15] = s["V"], s["ior"], s["dif"], s["opacity"]
                out[i, 16:19], out[i, 20:23] = s["spec"], s["emissive"]
            self._cache[key] = out
        return self._cache[key]

    def alpha_quantity(self, name):
        """the reading's alpha - threshold per record (its decision quantity), and its verdict"""
        r, sc = self.rec[name], self.reading
        q, fails = np.zeros(r.n), np.zeros(r.n, bool)
        for i in range(r.n):
            prim, u, v = int(r.prim[i]), float(r.uv[i, 0]), float(r.uv[i, 1])
            m = sc.mats[sc.mat_id[prim]]
            with np.errstate(all="ignore"):
                a = sc.sample_texture(m.texBaseColor, sc.tex_coord(prim, u, v), list(m.baseColor), (m.flags >> 3) & 7)[3]
                q[i] = a - m.alphaThreshold
            fails[i] = sc.alpha_test_fails(prim, u, v)
        return q, fails


_world = None


@pytest.fixture(scope="module")
def world(pkg, ob):
    global _world
    if _world is None:
        _world = World(pkg, ob)
    return _world


def deviations(orc, ref, rows, groups=es.GROUPS):
    """worst |oracle - reading| per field group over `rows`; a NaN on one side only counts as inf"""
    out = {}
    for g, cols in groups.items():
        a, b = orc[rows][:, cols].astype(np.float64), ref[rows][:, cols]
        with np.errstate(all="ignore"):
            d = np.abs(a - b)
            if g == "pos":
                d = d / np.maximum(1.0, np.abs(b))
        d = np.where(np.isnan(a) & np.isnan(b), 0.0, np.where(np.isnan(d), np.inf, d))
        d = np.where(np.isinf(a) & (a == b), 0.0, d)
        out[g] = float(d.max()) if d.size else 0.0
    return out


def _texture_rows(w, name):
    """rows of an addressing family whose texture-derived fields the float64 reading can be held against: |u * w| small
    enough that the fp32 product keeps its fraction"""
    r = w.rec[name]
    uv = w.sc.uv32(r.prim, r.uv[:, 0], r.uv[:, 1])
    return (np.abs(uv) < 1e3).all(axis=1)


WELL = ("ordinary", "texel_centres", "texel_edges", "seams", "last_texel", "far", "fraction_lost", "decode")


def measure_well(w, name, flags=0):
    orc, ref = w.oracle(name, flags), w.read(name, flags)
    rows = ~np.isnan(ref[:, 0:3]).any(axis=1)
    assert rows.all(), name
    dev = deviations(orc, ref, rows)
    tex = _texture_rows(w, name)
    dev["texture"] = deviations(orc, ref, rows & tex, {"texture": es.GROUPS["texture"]})["texture"]
    return dev, int(tex.sum())


@pytest.mark.parametrize("name", WELL)
def test_well_conditioned_family_within_its_bound(world, name):
    """every field of the record, oracle against the float64 reading, within four times the measured worst deviation"""
    dev, tex_rows = measure_well(world, name)
    print(name, dev, tex_rows)
    bound = es.BOUNDS[name]
    assert bound["texture"] < es.TEXTURE_LIMIT
    assert es.FAMILY_N - tex_rows == es.LEFT_OUT.get("texture/" + name, 0), (name, tex_rows)  # rows recorded only
    for g, d in dev.items():
        if g != "texture" or tex_rows:  # (no row to hold against float64: test_texel_pick_equals_the_fp32_restatement has them)
            assert d <= bound[g], (name, g, d, bound[g])


# ---- each family reaches its edge (fp32 restatement of the UV and fraction arithmetic) -----------------------------------
def _coords(w, name):
    """per record: shape (w, h) of its base texture and the fp32 (x, x0, fx), (y, y0, fy) of the sampler"""
    r = w.rec[name]
    uv = w.sc.uv32(r.prim, r.uv[:, 0], r.uv[:, 1])
    shape = np.array([w.sc.tex_shape[p // 2] for p in r.prim])
    return shape, texel32(uv[:, 0], shape[:, 0]), texel32(uv[:, 1], shape[:, 1]), uv


def test_addressing_families_reach_their_edges(world):
    w = world
    shape, (x, x0, fx), (y, y0, fy), uv = _coords(w, "texel_centres")
    assert (fx == 0).all() and (fy == 0).all()
    for s, (tw, th) in enumerate(es.SHAPES[:-1]):  # every column and row, the wrap column and row included
        m = (shape == (tw, th)).all(axis=1)
        assert set(x0[m]) == set(range(-1, tw + 1)) and set(y0[m]) == set(range(-1, th + 1)), (tw, th)
    assert ((x0 == 100) & (shape[:, 0] == 100)).any() and ((y0 == 37) & (shape[:, 1] == 37)).any()

    shape, (x, x0, fx), (y, y0, fy), uv = _coords(w, "texel_edges")
    assert (fx == 0.5).sum() > 40 and (fy == 0.5).sum() > 20
    for f in (fx, fy):  # one step of the UV either side of the half
        assert ((f > 0.5) & (f < 0.5001)).sum() > 10 and ((f < 0.5) & (f > 0.4999)).sum() > 10

    shape, _, _, uv = _coords(w, "seams")
    for c in (0.0, 1.0, -1.0, 2.0):
        for col in (0, 1):
            assert (uv[:, col] == F(c)).any() and (uv[:, col] == np.nextafter(F(c), F(np.inf))).any() and (uv[:, col] == np.nextafter(F(c), F(-np.inf))).any()

    shape, (x, x0, fx), (y, y0, fy), uv = _coords(w, "last_texel")
    assert (x0 == shape[:, 0] - 1).all() and (y0 == shape[:, 1] - 1).all()
    assert (fx == 0).any() and (fx > 0.99).any()

    shape, (x, x0, fx), (y, y0, fy), uv = _coords(w, "far")
    a = np.abs(uv)
    assert ((a > 3) & (a < 4.2)).any() and ((a > 8e3) & (a < 1.2e4)).any() and ((a > 8e6) & (a < 1.2e7)).any()
    assert (uv[:, 0] > 0).all() and (uv[:, 1] < 0).all()

    shape, (x, x0, fx), (y, y0, fy), uv = _coords(w, "fraction_lost")
    assert ((np.abs(x) >= 2 ** 23 - 1) & (np.abs(x) <= 2 ** 25)).all() and (fx == 0).all()
    assert (np.abs(y) >= 2 ** 23 - 1).sum() > 100

    shape, (x, x0, fx), (y, y0, fy), uv = _coords(w, "int_range")
    for c in (x, y):
        for sgn in (1, -1):
            assert (c == F(sgn * (INT_LIMIT - 128))).any() and (c == F(sgn * INT_LIMIT)).any() and (c == F(sgn * (INT_LIMIT + 256))).any()
            assert (np.abs(c - sgn * 1e12) < 1e6).any() and (c == sgn * np.inf).any()
        assert np.isnan(c).any() and (np.abs(c) > 1e38)[np.isfinite(c)].any()


def test_alpha_families_reach_their_ties(world):
    w = world
    r = w.rec["tie_const"]
    mats = [w.sc.mats[p // 2] for p in r.prim]
    alpha, thr = np.array([m.baseColor[3] for m in mats], F), np.array([m.alphaThreshold for m in mats], F)
    for t in es.CONST_THRESHOLDS:
        m = (thr == F(t)) & (np.signbit(thr) == np.signbit(F(t)))
        assert (alpha[m] == thr[m]).any() and (alpha[m] < thr[m]).any() and (alpha[m] > thr[m]).any(), t
        with np.errstate(all="ignore"):
            assert (np.abs(alpha[m].astype(np.float64) - t) <= np.spacing(np.abs(F(t)))).all() or t in (0.5, -1.0)
    assert np.isinf(thr).any() and np.isnan(thr).any()
    # flat textures: the four alpha bytes of every footprint are b and the threshold is b / 255 or a neighbour
    r = w.rec["tie_flat_texture"]
    on_tie = np.isin(r.prim // 2, w.sc.flat_cards)
    assert on_tie.sum() == es.FAMILY_N // 2
    seen = set()
    for p in r.prim[on_tie]:
        m = w.sc.mats[p // 2]
        t = w.sc.textures[m.texBaseColor][0]
        b = int(t[0, 0, 3])
        assert (t[..., 3] == b).all()
        k = [float(es.step(F(b) / F(255.0), s)) for s in (-1, 0, 1)].index(float(F(m.alphaThreshold)))
        seen.add((b, k))
    assert seen == {(b, k) for b in es.FLAT_BYTES for k in range(3)}
    shape, (x, x0, fx), (y, y0, fy), uv = _coords(w, "tie_bilinear")
    wide = shape[:, 0] == 2
    for f, m in ((fx, wide), (fy, ~wide)):
        assert (f[m] == 0.5).sum() >= 10 and ((f[m] > 0.5) & (f[m] < 0.50001)).any() and ((f[m] < 0.5) & (f[m] > 0.49999)).any()


# ---- the texel pick itself, against the fp32 restatement of the samplers ----------------------------------------------------
def _restated(w, name, flags=0):
    """per record of an addressing family: the columns of the record that are one bilinear sample of a LINEAR texture, and
    that sample from test_texel_fetch_exact.sample (fp32 numpy: floor, saturating conversion, wrap, pair load, blend)"""
    from test_texel_fetch_exact import sample
    r, sc = w.rec[name], w.sc
    uv = sc.uv32(r.prim, r.uv[:, 0], r.uv[:, 1])
    want, mask = np.zeros((r.n, 24), F), np.zeros((r.n, 24), bool)
    samples_tex = lambda typ, tid: typ not in (0, 1) and tid >= 0 and not sc.textures[tid][1]  # noqa: E731
    for k in np.unique(r.prim // 2):
        m, rows = sc.mats[k], np.flatnonzero(r.prim // 2 == k)
        with np.errstate(all="ignore"):
            if samples_tex((m.flags >> 3) & 7, m.texBaseColor) and m.flags & 7 != 0:  # spec-gloss: diffuse is the base colour
                want[rows, 12:15] = sample(sc.textures[m.texBaseColor][0], 0, uv[rows, 0], uv[rows, 1], new=True)[:, :3]
                mask[rows, 12:15] = True
            if samples_tex((m.flags >> 6) & 7, m.texSpecular) and m.flags & 7 != 0:  # specular rgb, roughness = max(0.08, 1 - a)
                t = sample(sc.textures[m.texSpecular][0], 0, uv[rows, 0], uv[rows, 1], new=True)
                lr = F(1.0) - t[:, 3]
                want[rows, 16:19], want[rows, 7] = t[:, :3], np.where(lr > F(0.08), lr, F(0.08))
                mask[rows, 16:19] = mask[rows, 7:8] = True
    return want, mask


@pytest.mark.parametrize("name", es.ADDRESS_FAMILIES)
def test_texel_pick_equals_the_fp32_restatement(world, name):
    """Every row of every addressing family, `far`, `fraction_lost`, `int_range` and `texcoord_range` included, where float64
    cannot follow: the fields that are one sample of a linear texture equal the numpy restatement of the sampler bit for
    bit (texel pick, wrap, fraction and blend; NaN where the coordinate is infinite or NaN)."""
    orc = world.oracle(name)
    want, mask = _restated(world, name)
    assert mask.any(axis=1).all(), name
    same = (orc.view(np.uint32) == want.view(np.uint32)) | (np.isnan(orc) & np.isnan(want)) | ~mask
    assert same.all(), (name, int((~same).any(axis=1).sum()))
    if name in ("fraction_lost", "int_range", "texcoord_range"):  # a whole texel, no blend: the value is one texel's
        shape, (x, x0, fx), (y, y0, fy), uv = _coords(world, name)
        whole = (fx == 0) & (fy == 0)
        assert whole.sum() >= {"fraction_lost": 120, "int_range": 25, "texcoord_range": 40}[name], int(whole.sum())


def test_texcoord_range_reaches_its_corners(world):
    """a corner hit returns the vertex's own texcoord bit for bit (where the triangle's other texcoords are finite), and the
    coordinates sit on the edges of the int range, infinite and NaN ones among them"""
    w = world
    r = w.rec["texcoord_range"]
    assert len(w.sc.range_tris) == 25 and set(tuple(s) for s in _coords(w, "texcoord_range")[0]) >= set(es.SHAPES)
    uv = w.sc.uv32(r.prim, r.uv[:, 0], r.uv[:, 1])
    T = w.sc.arrays.T[w.sc.I[r.prim]][:, :, :2]  # (n, 3 corners, 2)
    corner = np.where(r.uv[:, 0] == 1, 1, np.where(r.uv[:, 1] == 1, 2, 0))
    own = T[np.arange(r.n), corner]
    usable = np.isfinite(np.delete(T, 0, axis=1)).all(axis=(1, 2)) & (corner == 0) | np.isfinite(T).all(axis=(1, 2))
    assert usable.sum() >= 190
    assert ((uv.view(np.uint32) == own.view(np.uint32)) | (np.isnan(uv) & np.isnan(own)))[usable].all()
    assert np.isnan(uv[~usable]).all()  # 0 * inf
    shape, (x, x0, fx), (y, y0, fy), _ = _coords(w, "texcoord_range")
    c = np.concatenate([x, y])  # (a side that does not divide the target may have no fp32 texcoord whose product is exact)
    for sgn in (1, -1):
        for t in (INT_LIMIT - 128, INT_LIMIT, INT_LIMIT + 256):
            assert (c == F(sgn * t)).any(), (sgn, t)
        assert (c == sgn * np.inf).any() and (np.abs(c - sgn * 1e12) < 1e6).any()
    assert np.isnan(x).any() and np.isnan(y).any()


HOST_BUILDS = {"plain": (0.0, 0.0, 0), "split_and_clipped": (0.3, 1.0, 1)}


@pytest.mark.parametrize("build", list(HOST_BUILDS))
def test_host_trace_of_rays_straight_down(world, build):
    """The host build (its alpha clipping reads every vertex texcoord, the infinite and NaN ones of texcoord_range among
    them) and the host walk with AlphaClipper::testFails: the dyadic rays straight down, those onto the texcoord_range
    corners included, answer like the oracle's linear scan in all three modes, through the tree and through the host scan."""
    from test_refit_cpu import HostTree
    w = world
    rays = es.down_rays(w.sc)
    tree = HostTree(w.pkg, w.sc.desc, *HOST_BUILDS[build])
    for mode in (0, 1, 2):
        po, to = np.zeros(len(rays), np.int32), np.zeros((len(rays), 3), F)
        w.lib.oracle_trace(w.osc, rays.ctypes.data, len(rays), mode, 1, po.ctypes.data, to.ctypes.data)
        for brute in (0, 1):
            prim, tuv = tree.trace(rays, mode, brute)
            if mode == 2:
                assert np.array_equal(prim >= 0, po >= 0), (mode, brute, int(((prim >= 0) != (po >= 0)).sum()))
            else:
                assert np.array_equal(prim, po), (mode, brute, int((prim != po).sum()))
                assert np.array_equal(tuv.view(np.uint32), to.view(np.uint32)), (mode, brute)
    tree.close()
    # the corner rays meet both verdicts
    corner = (rays[:, 1] == 1) & (rays[:, 0] % 2 == 1) & np.isin((rays[:, 0] // 2).astype(int), [t // 2 for t in w.sc.range_tris])
    assert (po[corner] >= 0).any() and (po[corner] < 0).any()


# ---- ill-conditioned families: class only, outside the margin --------------------------------------------------------------
def _alpha_check(w, name):
    r = w.rec[name]
    q, fails = w.alpha_quantity(name)
    orc = w.ob.alpha_test(w.pkg.abi, w.osc, r.prim.astype(np.uint32), r.uv)
    # inside the margin: closer than MARGIN to the threshold without being on it.  An exact tie in the reading (a constant
    # alpha equal to the threshold, bytes 0 and 255 at fraction 0.5, alpha 0 against threshold 0) is a definite verdict,
    # "passes", and stays in; so does a NaN quantity, whose comparison is false in every precision.
    inside = (np.abs(q) < es.MARGIN) & (q != 0)
    return int(inside.sum()), int((orc != fails)[~inside].sum())


@pytest.mark.parametrize("name", es.ALPHA_FAMILIES + es.ADDRESS_FAMILIES[:4] + ("ordinary",))
def test_alpha_verdict_class(world, name):
    """oracle_alpha_test against the reading's alphaTestFails: the same verdict wherever the reading's alpha is further than
    the margin from the threshold"""
    inside, bad = _alpha_check(world, name)
    print(name, "inside the margin", inside, "differ", bad)
    assert bad == 0, (name, bad)
    assert inside == es.LEFT_OUT.get("alpha/" + name, 0) and inside <= es.FAMILY_N // 2, (name, inside)


def shading_margin(w, name, flags):
    """rows inside the margin of an ill-conditioned shading family, by the reading's own quantities"""
    r, ref = w.rec[name], w.read(name, flags)
    unread = np.isnan(ref[:, 0:3]).any(axis=1)  # the reading has no answer (a UV that is not finite, or beyond the int range)
    sc = w.reading
    small = lambda x: np.minimum(np.abs(x), 1.0 / np.maximum(np.abs(x), 1e-300)) < es.MARGIN  # noqa: E731
    with np.errstate(all="ignore"):
        b = np.stack([1.0 - r.uv[:, 0].astype(np.float64) - r.uv[:, 1], r.uv[:, 0], r.uv[:, 1]], axis=1)
        nsum = sc.n0[r.prim] * b[:, 0:1] + sc.n1[r.prim] * b[:, 1:2] + sc.n2[r.prim] * b[:, 2:3]
        inside = unread | small(np.linalg.norm(nsum, axis=1))        # the interpolated normal's length: 0, under- or overflow
        inside |= small(ref[:, 3])                                      # the distance to the origin
        inside |= np.abs(np.einsum("ij,ij->i", ref[:, 4:7], ref[:, 8:11])) < es.MARGIN  # N.V: the double-sided flip
        inside |= np.isnan(ref[:, 4:7]).any(axis=1)                     # a frame or map normal that is exactly 0 in float64
    return inside


def _shading_class_check(w, name, flags):
    orc, ref = w.oracle(name, flags), w.read(name, flags)
    inside = shading_margin(w, name, flags)
    keep = ~inside
    cols = [c for g in es.GROUPS.values() for c in g]
    nan_differs = (np.isnan(orc[:, cols]) != np.isnan(ref[:, cols])).any(axis=1)
    with np.errstate(all="ignore"):
        flipped = np.einsum("ij,ij->i", orc[:, 4:7].astype(np.float64), ref[:, 4:7]) < 0
    dev = deviations(orc, ref, keep)
    return int(inside.sum()), int((nan_differs & keep).sum()), int((flipped & keep).sum()), dev


ILL_SHADING = (("bary", 0), ("normals", 0), ("origin", 0), ("normal_map", NMAP), ("normal_map", 0), ("decode", NMAP), ("ordinary", NMAP))


@pytest.mark.parametrize("name,flags", ILL_SHADING)
def test_ill_conditioned_shading_class(world, name, flags):
    """outside the margin: the same fields are NaN, the normal points to the same side, and the values agree within the
    family's bound; inside: counted"""
    inside, nan_differs, flipped, dev = _shading_class_check(world, name, flags)
    print(name, flags, "inside the margin", inside, "NaN class differs", nan_differs, "flipped", flipped, dev)
    assert nan_differs == 0 and flipped == 0, (name, nan_differs, flipped)
    assert inside == es.LEFT_OUT.get(f"{name}/{flags}", 0) and inside <= es.FAMILY_N // 2, (name, inside)
    bound = es.BOUNDS[f"{name}/{flags}"]
    assert bound["texture"] < es.TEXTURE_LIMIT
    for g, d in dev.items():
        assert d <= bound[g], (name, g, d, bound[g])


def test_int_range_class(world):
    """rows whose u * w - 0.5 and v * h - 0.5 both stay inside the int range: the texture fields are finite and within the
    texture limit of SOME texel blend (each channel within the texture's range); beyond the range, and for NaN, the row is
    recorded only (the float64 reading's unbounded int is a third answer): the GPU test compares those with the oracle."""
    w = world
    shape, (x, x0, fx), (y, y0, fy), uv = _coords(w, "int_range")
    orc = w.oracle("int_range")
    with np.errstate(all="ignore"):
        inside_int = (np.abs(x) < INT_LIMIT) & (np.abs(y) < INT_LIMIT)
    tex = orc[:, es.GROUPS["texture"]]
    assert np.isfinite(tex[inside_int]).all()
    assert ((tex[inside_int] >= 0) & (tex[inside_int] <= 1)).all()
    beyond = int((~inside_int).sum())
    print("int_range: beyond the int range or NaN", beyond, "of", len(x))
    assert beyond == es.LEFT_OUT["int_range"]
    # a NaN coordinate makes the fraction NaN: every texture field of those rows is NaN, in any conversion rule; the
    # roughness is maxf(0.08, NaN) = 0.08
    nan_rows = np.isnan(x) | np.isnan(y)
    assert nan_rows.sum() > 10 and np.isnan(tex[nan_rows][:, 1:]).all() and (tex[nan_rows][:, 0] == F(0.08)).all()


def test_flat_texture_alpha_is_the_bytes_value(world):
    """tie_flat_texture: whatever the fraction, the bilinear sum of four equal alpha bytes b is fp32(b / 255.0f) exactly
    (the differences are 0), so the candidate fails only against the threshold one step above that value."""
    w = world
    r = w.rec["tie_flat_texture"]
    on_tie = np.isin(r.prim // 2, w.sc.flat_cards)
    fails = w.ob.alpha_test(w.pkg.abi, w.osc, r.prim.astype(np.uint32), r.uv)
    expect = np.zeros(r.n, bool)
    for i in np.flatnonzero(on_tie):
        m = w.sc.mats[r.prim[i] // 2]
        b = w.sc.textures[m.texBaseColor][0][0, 0, 3]
        expect[i] = F(b) / F(255.0) < F(m.alphaThreshold)
    assert 20 < expect.sum() < on_tie.sum()
    assert np.array_equal(fails[on_tie], expect[on_tie]), int((fails != expect)[on_tie].sum())


# ---- the two predicted divergences, named ----------------------------------------------------------------------------------
def test_oracle_samples_types_3_to_7_at_the_hit_uv(world):
    """Diffuse channel types 3 .. 7 with a texture: the alpha test samples at the hit's UV, as sampleTexture and
    prepareShadingData do (the oracle's alphaTestFails sampled at (0, 0) before: alpha 1 there, 0 at these hits)."""
    w = world
    r = w.rec["types_3_to_7"]
    away = ~(r.uv == 0).all(axis=1)
    fails = w.ob.alpha_test(w.pkg.abi, w.osc, r.prim.astype(np.uint32), r.uv)
    types = np.array([(w.sc.mats[p // 2].flags >> 3) & 7 for p in r.prim])
    assert set(types) == {3, 4, 5, 6, 7}
    assert fails[away].all() and not fails[~away].any(), (int(fails[away].sum()), int(away.sum()))


def test_oracle_float_to_int_saturates(world):
    """Beyond the int range the samplers convert as the device's convert instruction does: saturating, NaN -> 0.  The rows
    of int_range beyond +-2^31 must pick the texels of INT_MAX / INT_MIN under wrap addressing, with fraction 0 (x is then
    an integer), or NaN where x is infinite (inf - inf)."""
    w = world
    shape, (x, x0, fx), (y, y0, fy), uv = _coords(w, "int_range")
    r = w.rec["int_range"]
    orc = w.oracle("int_range")
    sat = lambda c: np.where(np.isnan(c), 0, np.clip(np.nan_to_num(c.astype(np.float64), nan=0.0, posinf=INT_LIMIT, neginf=-INT_LIMIT), -INT_LIMIT, INT_LIMIT - 1)).astype(np.int64)  # noqa: E731
    with np.errstate(all="ignore"):
        rows = np.flatnonzero(((np.abs(x) >= INT_LIMIT) | (np.abs(y) >= INT_LIMIT)) & np.isfinite(x) & np.isfinite(y))
    assert len(rows) > 60
    ix, iy = sat(x0) % shape[:, 0], sat(y0) % shape[:, 1]
    checked = 0
    for i in rows:
        if fx[i] != 0 or fy[i] != 0:
            continue  # (the other coordinate is an ordinary one: a blend)
        m = w.sc.mats[r.prim[i] // 2]
        t = w.sc.textures[m.texSpecular][0]  # the linear copy: specular rgb = bytes / 255
        expect = t[iy[i], ix[i], :3].astype(F) / F(255.0)
        assert np.array_equal(orc[i, 16:19], expect), (i, x[i], y[i], orc[i, 16:19], expect)
        checked += 1
    assert checked > 20


if __name__ == "__main__":
    import __graft_entry__ as ge
    import oracle_binding
    package = ge.load_package()
    wd = World(package, oracle_binding)
    fmt = lambda d: "{" + ", ".join(f'"{g}": {x:.1e}' for g, x in d.items()) + "}"  # noqa: E731
    left = {}
    print("MEASURED = {")
    for nm in WELL:
        dev, rows = measure_well(wd, nm)
        if rows != es.FAMILY_N:
            left["texture/" + nm] = es.FAMILY_N - rows
        print(f'    "{nm}": {fmt(dev)},')
    for nm, fl in ILL_SHADING:
        inside, nan_differs, flipped, dev = _shading_class_check(wd, nm, fl)
        left[f"{nm}/{fl}"] = inside
        print(f'    "{nm}/{fl}": {fmt(dev)},  # NaN class differs {nan_differs}, flipped {flipped}')
    print("}")
    for nm in es.ALPHA_FAMILIES + es.ADDRESS_FAMILIES[:4] + ("ordinary",):
        inside, bad = _alpha_check(wd, nm)
        if inside:
            left["alpha/" + nm] = inside
        print(f"# alpha/{nm}: inside the margin {inside}, verdicts that differ outside it {bad}")
    xy = _coords(wd, "int_range")
    with np.errstate(all="ignore"):
        left["int_range"] = int((~((np.abs(xy[1][0]) < INT_LIMIT) & (np.abs(xy[2][0]) < INT_LIMIT))).sum())
    print("LEFT_OUT =", left)
