"""Edge-case surface records for the hit-shading and alpha-test tests (tests/test_surface_edge_records_cpu.py,
tests/test_gpu_surface_edge_records.py): one small scene and named families of (prim, u, v, ray origin) records that no
frame produces.  Seeded, plain numpy; no product code.

The scene (EdgeScene) is a row of unit quads in the plane z = 0.  Quad k covers [2k, 2k+1] x [0, 1], has four vertices
and one material of its own and two triangles with three vertices each: A = (v0, v1, v3), prim 2k, and B = (v2, v3, v1),
prim 2k + 1.  The texture coordinates are the position within the quad, (0,0) (1,0) (1,1) (0,1).  On triangle A two of
them are zero in either component, so a hit (prim 2k, u, v) has the fp32 texture coordinate (u, v) bit for bit, whatever u
and v are: the families put any UV they need into the barycentrics, as a caller's hit may.  Barycentrics far outside the
triangle cancel in the interpolated normal, so the families `far` and `fraction_lost` use triangle B of the addressing
quads instead, whose texture coordinates are (0,0) (2^24,0) (0,-2^24): a hit inside it has the exact UV (2^24 u, -2^24 v).
A ray straight down from a dyadic (x, y) has exact barycentrics on either triangle.  EdgeScene(bare=True) is the second,
tiny scene: no texcoords, no bitangents, materials that ask for textures and normal maps.  The quads stand in the order
normal map, interpolation and view, decode, alpha cards, addressing; the camera of view "start" looks down the row from
its first quad, that of "end" back from its last.

Textures: every shape of SHAPES as an sRGB and a linear copy; neighbouring texels (the wrap neighbours included) differ by
at least 32/255 in every channel, and together the textures hold the EDGE_BYTES of test_gpu_walk_lds_tables.py.

  family            what it is for
  ordinary          random hits inside both triangles of every quad, the origin above or below
  texel_centres     u * w - 0.5 an exact integer (fx = fy = 0): every column and row of the shapes up to 8 texels, the wrap
                    column and row included; a stride over 100 x 37
  texel_edges       fx = 0.5 exactly (fy likewise) and one fp32 step of the UV either side
  seams             u, v in {0, 1, -1, 2}, and one step either side
  last_texel        the footprint of texel (w - 1, h - 1): the pair load's spare texel, the wrap column's own load
  far               |uv| around 3.7, 1e4 and 1e7
  fraction_lost     |u * w| from 2^23 to 2^25: the product has no fraction bits left
  int_range         u * w - 0.5 at +-(2^31 - 128), +-2^31, +-(2^31 + 256), +-1e12, +-3e38 (w = 1) or +-inf, and NaN, reached
                    through the barycentrics (any texcoord a vertex could carry, a caller's hit can produce)
  texcoord_range    the same values as vertex texcoords: the second triangles of the textured alpha cards (25 triangles, every
                    shape) carry them, one corner each, and are hit at that corner; infinite and NaN texcoords among them
  bary              barycentrics on corners and edges, u + v one step above 1, outside the triangle, NaN and inf
  normals           quads whose vertex normals are opposite, all zero, of length 1e-3, 1e3, 1e-25, 1e20, or signed zeros
  origin            the origin at posW, in the tangent plane and one step either side, behind a single- and a
                    double-sided surface, 1e-20 and 1e20 away
  decode            every decode material at ordinary hits: metalness 0 / 0.5 / 1, roughness around the 0.08 clamp as a
                    factor and from bytes 20 / 21, gloss 0 / 1 / 2, a NaN roughness factor, all eight values of the three
                    channel types with and without a texture (TEXTURE with id -1 among them), shading models 0 .. 7
  normal_map        map texels (128,128,255), (0,0,.), (255,255,.), the midpoint of 127 and 128; types 0 .. 3 with and
                    without a texture; bitangents parallel to N, zero and non-unit
  tie_const         constant alpha equal to the threshold and one step either side; thresholds 0, -0, 1, 2, -1, inf, NaN
  tie_flat_texture  all alpha bytes b in {0, 1, 127, 128, 254, 255}, threshold fp32(b / 255.0f) and its neighbours, any
                    fraction: the bilinear sum must return the byte's value exactly
  tie_bilinear      alpha bytes (0, 255) in a 2 x 1 and a 1 x 2 texture, threshold 0.5, fx / fy 0.5 and a step either side
  unused            diffuse type UNUSED (alpha 0) with threshold 0 (passes) and the smallest subnormal (fails)
  types_3_to_7      diffuse types 3 .. 7 with a texture whose alpha at (0, 0) differs from its alpha elsewhere

Measured on the CPU: the oracle (fp32) against the float64 reading (tests/hlsl_textured_numpy.py), FAMILY_N = 256 records
per family, worst absolute deviation per field group over the rows compared (MEASURED below; `python
tests/test_surface_edge_records_cpu.py` prints it).  The asserted bound of a well-conditioned family is four times the
measured worst, rounded up to one digit (BOUNDS); every texture-derived bound stays below TEXTURE_LIMIT = 1 / (2 * 255).
"class" families are ill-conditioned: oracle and reading must agree in class (pass / fail, flipped / not, finite / NaN)
outside a margin of MARGIN = 1e-6 in the reading's own decision quantity; LEFT_OUT is how many rows sit inside it.
An exact tie in the reading (alpha == threshold) is a definite verdict and stays outside the margin.
Where float64 cannot follow — `far` beyond 1e3, `fraction_lost`, `int_range`, `texcoord_range`: the fp32 product u * w
is rounded by whole texels or leaves the int range — the texture-derived fields are held bit for bit against the fp32
numpy restatement of the sampler instead (test_texel_pick_equals_the_fp32_restatement, every row of every addressing
family); "texture/<family>" in LEFT_OUT counts those rows, and a texture figure of 0 in MEASURED over no row asserts nothing.
"""
import numpy as np

from area_scenes import DescArrays
from edge_records import Batch, F, FAMILY_N, _interleave, step

SHAPES = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (8, 8), (8, 4), (5, 8), (100, 37))  # (w, h)
EDGE_BYTES = (0, 10, 11, 1, 9, 12, 127, 128, 254, 255)  # test_gpu_walk_lds_tables.py
MARGIN = 1e-6
TEXTURE_LIMIT = 1.0 / (2 * 255)
UV_SCALE = 2.0 ** 24
TINY = F(1e-45)  # the smallest subnormal
FLAT_BYTES = (0, 1, 127, 128, 254, 255)
CONST_THRESHOLDS = (0.0, -0.0, 1.0, 2.0, -1.0)

# field groups of a bdpt_surface record (columns of the (n, 24) float32 array)
GROUPS = {"pos": [0, 1, 2, 3], "N": [4, 5, 6], "V": [8, 9, 10], "factor": [11, 15], "texture": [7, 12, 13, 14, 16, 17, 18, 20, 21, 22]}

# family (ill-conditioned ones: "family/shade flags", over the rows outside the margin) -> worst |oracle - float64 reading| per
# group, measured (see the module docstring); pos is relative to max(1, |x|)
MEASURED = {
    "ordinary": {"pos": 5.2e-06, "N": 9.2e-08, "V": 1.6e-05, "factor": 0.0e+00, "texture": 6.7e-07},
    "texel_centres": {"pos": 9.1e-06, "N": 0.0e+00, "V": 2.4e-05, "factor": 0.0e+00, "texture": 2.7e-06},
    "texel_edges": {"pos": 1.1e-05, "N": 0.0e+00, "V": 1.7e-05, "factor": 0.0e+00, "texture": 1.4e-06},
    "seams": {"pos": 2.0e-05, "N": 0.0e+00, "V": 3.4e-05, "factor": 0.0e+00, "texture": 4.6e-06},
    "last_texel": {"pos": 1.9e-05, "N": 0.0e+00, "V": 4.4e-05, "factor": 0.0e+00, "texture": 3.1e-06},
    "far": {"pos": 1.2e-05, "N": 0.0e+00, "V": 1.4e-05, "factor": 0.0e+00, "texture": 9.4e-06},
    "fraction_lost": {"pos": 2.2e-05, "N": 0.0e+00, "V": 2.3e-05, "factor": 0.0e+00, "texture": 0.0e+00},
    "decode": {"pos": 2.8e-06, "N": 0.0e+00, "V": 5.6e-06, "factor": 0.0e+00, "texture": 2.3e-07},
    "bary/0": {"pos": 8.9e-08, "N": 0.0e+00, "V": 9.2e-08, "factor": 0.0e+00, "texture": 8.1e-07},
    "normals/0": {"pos": 1.3e-06, "N": 9.2e-08, "V": 2.5e-06, "factor": 0.0e+00, "texture": 1.2e-09},
    "origin/0": {"pos": 1.2e-06, "N": 0.0e+00, "V": 3.2e-06, "factor": 0.0e+00, "texture": 1.2e-09},
    "normal_map/1": {"pos": 4.2e-07, "N": 1.6e-07, "V": 9.6e-07, "factor": 0.0e+00, "texture": 1.2e-09},
    "normal_map/0": {"pos": 5.3e-07, "N": 0.0e+00, "V": 9.6e-07, "factor": 0.0e+00, "texture": 1.2e-09},
    "decode/1": {"pos": 2.8e-06, "N": 0.0e+00, "V": 5.6e-06, "factor": 0.0e+00, "texture": 2.3e-07},
    "ordinary/1": {"pos": 5.2e-06, "N": 9.2e-08, "V": 1.6e-05, "factor": 0.0e+00, "texture": 6.7e-07},
}


def bound_of(measured):
    """four times the measured worst deviation, rounded up to one digit"""
    x = 4.0 * measured
    if x == 0:
        return 0.0
    e = np.floor(np.log10(x))
    return float(np.ceil(x / 10 ** e * (1 - 1e-12)) * 10 ** e)


# rows inside the margin (ill-conditioned families: "family/shade flags", "alpha/family") or recorded only ("texture/family",
# "int_range"), of FAMILY_N
LEFT_OUT = {
    "texture/far": 220,
    "texture/fraction_lost": 256,
    "bary/0": 64,
    "normals/0": 126,
    "origin/0": 96,
    "normal_map/1": 67,
    "alpha/tie_const": 69,
    "alpha/tie_flat_texture": 113,
    "alpha/tie_bilinear": 86,
    "alpha/unused": 64,
    "alpha/ordinary": 80,
    "int_range": 230,
}
BOUNDS = {k: {g: bound_of(x) for g, x in v.items()} for k, v in MEASURED.items()}


def flags(model=0, dif=1, spec=1, emis=1, nmap=0, alpha=0, dbl=0):
    return model | (dif << 3) | (spec << 6) | (emis << 9) | (nmap << 12) | (alpha << 17) | (dbl << 19)


def texture(w, h, seed):
    """(h, w, 4) uint8: byte = (a_c + mx * x + my * y) mod 256 with steps whose every neighbour difference, the wrap
    neighbour's included, is at least 32"""
    ok = lambda m, n: 32 <= m <= 224 and (n <= 2 or 32 <= (m * (n - 1)) % 256 <= 224)  # noqa: E731
    rng = np.random.default_rng(seed)
    mx = next(m for m in rng.permutation(np.arange(33, 224, 2)) if ok(int(m), w))
    my = next(m for m in rng.permutation(np.arange(33, 224, 2)) if ok(int(m), h) and m != mx)
    a = rng.integers(0, 256, 4)
    y, x = np.mgrid[0:h, 0:w]
    t = ((a[None, None, :] + int(mx) * x[..., None] + int(my) * y[..., None]) % 256).astype(np.uint8)
    for axis, n in ((1, w), (0, h)):
        if n > 1:
            assert (np.abs(t.astype(int) - np.roll(t, -1, axis=axis).astype(int)) >= 32).all(), (w, h)
    return t


def _mat(a, fl, base=(0.75, 0.5, 0.25, 1.0), spec=(0.5, 0.5, 0.25, 0.5), emis=(0.125, 0.25, 0.5), thr=0.5, tb=-1, ts=-1, te=-1, tn=-1):
    m = a.Material()
    m.baseColor[:], m.specular[:], m.emissive[:] = base, spec, emis
    m.alphaThreshold, m.IoR, m.flags = thr, 1.5, fl
    m.texBaseColor, m.texSpecular, m.texEmissive, m.texNormal = tb, ts, te, tn
    return m


Z = (0.0, 0.0, 1.0)


class EdgeScene:
    """The row of quads.  quads: name -> quad index (or a list of them); tex_shape[k]: the (w, h) of quad k's base-colour
    texture, or None.  finite=True leaves out the quads whose shading is NaN or infinite at ordinary hits (for frames);
    ceiling=True adds one large double-sided quad at z = 2 over the whole row (for walks of more than one step)."""

    def __init__(self, abi, bare=False, finite=False, view="start", ceiling=False):
        self.abi, self.bare, self.view, self.finite = abi, bare, view, finite
        self.textures, self.mats, self.vn, self.vb, self.tex_shape, self.quads = [], [], [], [], [], {}
        tex = self._tex
        if bare:
            t = tex(texture(3, 5, 1), True)
            nm = tex(self._nmap_texture(), False)
            self._quad("bare_rgb", _mat(abi, flags(2, 2, 2, 2, nmap=1, alpha=1, dbl=1), tb=t, ts=t, te=t, tn=nm), shape=(3, 5))
            self._quad("bare_rg", _mat(abi, flags(0, 2, 2, 2, nmap=2, dbl=0), tb=t, ts=t, te=t, tn=nm), shape=(3, 5))
            self._finish(texcoords=False, bitangents=False)
            return
        # -- the addressing textures (their quads come last in the row, next to the "end" camera)
        self.addr_tex = []
        for s, (w, h) in enumerate(SHAPES):
            lin = texture(w, h, 100 + s)
            if w * h == 1:
                lin[..., 3] = 200  # (a 1 x 1 card below its threshold would be dropped by the build's alpha clipping)
            self.addr_tex.append((tex(lin.copy(), True), tex(lin, False)))
        used = set(np.unique(np.concatenate([t.reshape(-1) for t, _ in self.textures])))
        assert set(EDGE_BYTES) <= used
        # -- normal map
        nm = tex(self._nmap_texture(), False)
        nmk = {f"type_{t}": dict(fl=flags(nmap=t, dbl=1), tn=nm) for t in range(4)}
        nmk.update({f"type_{t}_none": dict(fl=flags(nmap=t, dbl=1)) for t in (1, 2)})
        for k, bt in (("bit_parallel", [Z] * 4), ("bit_zero", [(0, 0, 0)] * 4), ("bit_nonunit", [(0.0, 250.0, 1.0)] * 4)):
            nmk[k] = dict(fl=flags(nmap=1, dbl=1), tn=nm, bt=bt)
        self.nmap_kinds = tuple(k for k in nmk if not (finite and k in ("bit_parallel", "bit_zero")))
        for k in self.nmap_kinds:
            kw = dict(nmk[k])
            bt = kw.pop("bt", None)
            self._quad(("nmap", k), _mat(abi, kw.pop("fl"), **kw), bitangents=bt, shape=(8, 1))
        # -- interpolation and view
        self._quad("plain_ds", _mat(abi, flags(dbl=1)))
        self._quad("plain_ss", _mat(abi, flags(dbl=0)))
        tilt = np.array([0.6, 0.0, 0.8])
        nrm = {"opposite": [Z, (0, 0, -1), (0, 0, -1), Z], "zero": [(0, 0, 0)] * 4,
               "len_1e-3": [tilt * 1e-3] * 4, "len_1e3": [tilt * 1e3] * 4, "len_1e-25": [tilt * 1e-25] * 4, "len_1e20": [tilt * 1e20] * 4,
               "signed_zero": [(-0.0, 0.0, 1.0), (0.0, -0.0, 1.0), (-0.0, -0.0, 1.0), (-0.0, -0.0, -1.0)]}
        self.normal_kinds = tuple(nrm)
        for k, v in nrm.items():
            if not (finite and k in ("opposite", "zero", "len_1e-25", "len_1e20", "signed_zero")):
                self._quad(("normals", k), _mat(abi, flags(dbl=1)), normals=v)
        # -- material decode
        rb = np.zeros((1, 2, 4), np.uint8)
        rb[0, 0], rb[0, 1] = (200, 20, 40, 255), (100, 21, 200, 90)
        rough_bytes = tex(rb, False)
        dec = {"metal_0_rough_below": dict(fl=flags(0, dbl=1), spec=(0.3, 0.07, 0.0, 0.3)),
               "metal_half_rough_at": dict(fl=flags(0, dbl=1), spec=(0.3, 0.08, 0.5, 0.3)),
               "metal_1_rough_above": dict(fl=flags(0, dbl=1), spec=(0.3, 0.09, 1.0, 0.3)),
               "rough_bytes": dict(fl=flags(0, 1, 2, 1, dbl=1), ts=rough_bytes, shape=(2, 1)),
               "gloss_0": dict(fl=flags(2, dbl=1), spec=(0.5, 0.25, 0.125, 0.0)),
               "gloss_1": dict(fl=flags(2, dbl=1), spec=(0.5, 0.25, 0.125, 1.0)),
               "gloss_2": dict(fl=flags(2, dbl=1), spec=(0.5, 0.25, 0.125, 2.0)),
               "rough_nan": dict(fl=flags(0, dbl=1), spec=(0.3, np.nan, 0.25, 0.3))}
        t35 = self.addr_tex[4]
        for t in range(8):  # each of the four fields takes every value once, and no two of them the same value in one material
            fl = flags(t, (t + 2) % 8, (t + 5) % 8, (t + 7) % 8, dbl=1)
            dec[f"type_{t}_tex"] = dict(fl=fl, tb=t35[0], ts=t35[1], te=t35[0], shape=SHAPES[4])
            dec[f"type_{t}_none"] = dict(fl=fl)
        self.decode_kinds = tuple(k for k in dec if not (finite and k == "rough_nan"))
        for k in self.decode_kinds:
            kw = dict(dec[k])
            self._quad(("decode", k), _mat(abi, kw.pop("fl"), **{a_: b_ for a_, b_ in kw.items() if a_ != "shape"}), shape=kw.get("shape"))
        # -- alpha
        self.const_cards = []
        for thr in CONST_THRESHOLDS:
            for k in (-1, 0, 1):
                alpha = float(step(F(thr), k)) if thr != 0 else float((TINY * k if k else F(thr)))
                self.const_cards.append(self._quad(("tie_const", str(thr), k), _mat(abi, flags(alpha=1, dbl=1), base=(0.5, 0.5, 0.5, alpha), thr=thr)))
        for thr, alpha in () if finite else ((np.inf, np.inf), (np.inf, 3e38), (np.nan, 1.0), (np.nan, np.nan)):
            self.const_cards.append(self._quad(("tie_const", str(thr), str(alpha)), _mat(abi, flags(alpha=1, dbl=1), base=(0.5, 0.5, 0.5, alpha), thr=thr)))
        self.flat_cards = []
        for b in FLAT_BYTES:
            for k in (-1, 0, 1):  # (a shape of SHAPES each: the cards' second triangles carry the texcoord_range corners)
                w, h = SHAPES[len(self.flat_cards) % len(SHAPES)]
                t = texture(w, h, 200 + len(self.flat_cards))
                t[..., 3] = b
                thr = float(step(F(b) / F(255.0), k))
                self.flat_cards.append(self._quad(("tie_flat", b, k), _mat(abi, flags(1, 2, alpha=1, dbl=1), tb=tex(t, False), thr=thr), shape=(w, h)))
        self.bilinear_cards = []
        for w, h in ((2, 1), (1, 2)):
            t = texture(w, h, 300 + w)
            t[..., 3].reshape(-1)[:] = (0, 255)
            self.bilinear_cards.append(self._quad(("tie_bilinear", w), _mat(abi, flags(1, 2, alpha=1, dbl=1), tb=tex(t, False), thr=0.5), shape=(w, h)))
        self.unused_cards = [self._quad(("unused", 0), _mat(abi, flags(1, 0, alpha=1, dbl=1), thr=0.0)),
                             self._quad(("unused", 1), _mat(abi, flags(1, 0, alpha=1, dbl=1), thr=float(TINY)))]
        self.clear_cards = [self._quad(("unused", 2), _mat(abi, flags(1, 0, alpha=1, dbl=1), thr=0.5)),   # alpha 0: fails, well clear
                            self._quad(("unused", 3), _mat(abi, flags(1, 0, alpha=1, dbl=1), thr=-1.0))]  # passes
        t = texture(5, 3, 400)
        t[..., 3] = 0
        t[0, 0, 3] = t[0, 4, 3] = t[2, 0, 3] = t[2, 4, 3] = 255  # the footprint of uv = (0, 0)
        tid = tex(t, False)
        self.type_cards = [self._quad(("types_3_to_7", ty), _mat(abi, flags(1, ty, alpha=1, dbl=1), base=(0.5, 0.5, 0.5, 0.25), tb=tid, thr=0.5), shape=(5, 3))
                           for ty in (3, 4, 5, 6, 7)]
        # -- texture addressing: spec-gloss, base and emissive from the sRGB copy, specular and gloss from the linear one;
        # alpha-tested at 0.5, so the same records serve the alpha tests
        for s, (w, h) in enumerate(SHAPES):
            ts, tl = self.addr_tex[s]
            self._quad(("addr", s), _mat(abi, flags(2, 2, 2, 2, alpha=1, dbl=1), tb=ts, ts=tl, te=ts), shape=(w, h))
        if ceiling:  # (for walks of more than one step: one large quad over the whole row, placed by _finish)
            self._quad("ceiling", _mat(abi, flags(dbl=1)))
        self._finish()

    @staticmethod
    def _nmap_texture():
        t = np.zeros((1, 8, 4), np.uint8)
        t[0] = [(128, 128, 255, 255), (0, 0, 200, 255), (255, 255, 40, 255), (127, 127, 127, 255), (128, 128, 128, 255),
                (128, 128, 255, 255), (0, 0, 200, 255), (255, 255, 40, 255)]
        return t

    def _tex(self, t, srgb):
        self.textures.append((np.ascontiguousarray(t), srgb))
        return len(self.textures) - 1

    def _quad(self, name, mat, normals=None, bitangents=None, shape=None):
        k = len(self.mats)
        self.mats.append(mat)
        self.vn.append(np.array(normals if normals is not None else [Z] * 4, np.float64))
        self.vb.append(np.array(bitangents if bitangents is not None else [(0.0, 1.0, 0.0)] * 4, np.float64))
        self.tex_shape.append(shape)
        assert name not in self.quads
        self.quads[name] = k
        return k

    def _finish(self, texcoords=True, bitangents=True):
        a, nq = self.abi, len(self.mats)
        corner = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], F)
        order = [0, 1, 3, 2, 3, 1]  # six vertices per quad: A = (v0, v1, v3), B = (v2, v3, v1)
        P = np.concatenate([corner[order] + np.array([2 * k, 0, 0], F) for k in range(nq)]).astype(F)
        T = np.tile(corner[order], (nq, 1)).astype(F)
        if "ceiling" in self.quads:
            k = self.quads["ceiling"]
            P[6 * k: 6 * k + 6] = (corner[order] * np.array([2 * nq + 8, 8, 0], F) + np.array([-4, -4, 2], F)).astype(F)
        for k in self.quad_list("addr"):  # B of an addressing quad: (0, 0), (UV_SCALE, 0), (0, -UV_SCALE)
            T[6 * k + 3: 6 * k + 6] = [(0, 0, 0), (UV_SCALE, 0, 0), (0, -UV_SCALE, 0)]
        # texcoord_range: the second triangles of the textured alpha cards carry texcoords whose u * w - 0.5 sits on the
        # edges of the int range, one corner each; every third triangle has one corner that is not finite (its other two
        # corners then interpolate to NaN: 0 * inf) and the rest have three finite ones
        self.range_tris, self.range_target = [], {}
        if texcoords and not self.finite and not self.bare:
            signed = [(t, sgn) for t in INT_RANGE_TARGETS for sgn in (1, -1)]
            fin = [c for c in signed if np.isfinite(c[0])]
            non = [c for c in signed if not np.isfinite(c[0])]
            for j, k in enumerate(self.flat_cards + self.type_cards + self.bilinear_cards):
                w, h = self.tex_shape[k]
                for c in range(3):
                    pick = non if (j % 3 == 0 and c == 0) else fin
                    tu, tv = pick[(3 * j + c) % len(pick)], pick[(5 * j + 2 * c + 1) % len(pick)]
                    T[6 * k + 3 + c] = (texcoord_for(*tu, w), texcoord_for(*tv, h), 0)
                    self.range_target[(2 * k + 1, c)] = (tu, tv)
                self.range_tris.append(2 * k + 1)
        I = np.arange(6 * nq, dtype=np.uint32).reshape(-1, 3)
        M = np.repeat(np.arange(nq, dtype=np.uint32), 2)
        with np.errstate(all="ignore"):
            N = np.concatenate([v[order] for v in self.vn]).astype(F)
            B = np.concatenate([v[order] for v in self.vb]).astype(F)
        lt = a.Light()
        lt.type = a.LIGHT_POINT
        lt.posW[:], lt.dirW[:], lt.intensity[:] = (float(nq), 0.5, 4.0), (0.0, 0.0, -1.0), (40.0, 40.0, 40.0)
        lt.openingAngle, lt.cosOpeningAngle, lt.penumbraAngle = np.pi, -1.0, 0.0
        self.nq = nq
        self.arrays = DescArrays(a, P, N, T if texcoords else np.zeros_like(T), I, M, self.mats, self.textures, [lt], B=B if bitangents else None)
        if not texcoords:
            self.arrays.desc.texcoords = None
        self.desc, self.P, self.I = self.arrays.desc, P, I
        assert 2 * nq < 200
        # quads whose shading is well-conditioned at ordinary hits
        odd = [self.quads[n] for n in self.quads if isinstance(n, tuple) and n[0] == "normals" and n[1] not in ("len_1e-3", "len_1e3")]
        odd += [self.quads[("nmap", n)] for n in ("bit_parallel", "bit_zero") if ("nmap", n) in self.quads]
        odd += [self.quads["ceiling"]] if "ceiling" in self.quads else []
        self.ordinary_quads = np.array([k for k in range(nq) if k not in odd])
        self.a_only = np.array(self.quad_list("addr") + [t // 2 for t in self.range_tris])  # ordinary hits keep to triangle A there

    def camera(self, aspect):
        """down the row from beyond its first quad (view "start") or back from beyond its last (view "end"): the row is 1 wide,
        so a frame holds a dozen quads at a size worth shading and the rest as a thin line"""
        cam = self.abi.Camera()
        sgn = 1.0 if self.view == "start" else -1.0
        f = np.array([sgn, 0.0, -0.7])
        f /= np.linalg.norm(f)
        right = np.array([0.0, -sgn, 0.0])
        up = np.cross(right, f)
        cam.posW[:] = (-2.0 if self.view == "start" else 2.0 * self.nq + 1.0, 0.5, 4.0)
        cam.cameraU[:], cam.cameraV[:], cam.cameraW[:] = tuple(right * 0.1), tuple(up * 0.65), tuple(f)
        return cam

    def quad_list(self, prefix):
        return [k for n, k in self.quads.items() if isinstance(n, tuple) and n[0] == prefix]

    # ---- the fp32 restatements the families check themselves with (operation order of device_scene.hpp shadeHitLut)
    def pos32(self, prim, bu, bv):
        with np.errstate(all="ignore"):
            b0 = (F(1.0) - bu) - bv
            p = self.P[self.I[prim]]  # (n, 3 vertices, 3)
            return ((p[:, 0] * b0[:, None] + p[:, 1] * bu[:, None]) + p[:, 2] * bv[:, None]).astype(F)

    def uv32(self, prim, bu, bv):
        with np.errstate(all="ignore"):
            b0 = (F(1.0) - bu) - bv
            t = self.arrays.T[self.I[prim]]
            return (((F(0) + t[:, 0] * b0[:, None]) + t[:, 1] * bu[:, None]) + t[:, 2] * bv[:, None]).astype(F)[:, :2]


def texel32(u, n):
    """(x, floor(x), fraction) of the samplers' u * n - 0.5 in fp32 (test_texel_fetch_exact.sample has the same lines)"""
    with np.errstate(all="ignore"):
        x = np.asarray(u, F) * F(n) - F(0.5)
        x0 = np.floor(x)
        return x, x0, (x - x0).astype(F)


def _solve(target_x, n, frac=0.0):
    """a u whose fp32 u * n - 0.5 is exactly target_x + frac, or None"""
    u0 = F((target_x + frac + 0.5) / n)
    for k in (0, 1, -1, 2, -2, 3, -3, 4, -4):
        u = step(u0, k)[()] if k else u0
        if texel32(u, n)[0] == F(target_x + frac):
            return F(u)
    return None


class SurfaceRecords(Batch):
    """prim (n,) int32, uv (n, 2) barycentrics, org (n, 3); rays / hits in the layouts of bdpt_ray / bdpt_hit"""

    def __init__(self, d, family, names):
        super().__init__(family, names)
        self.prim, self.uv, self.org = np.ascontiguousarray(d["prim"], np.int32), np.ascontiguousarray(d["uv"], F), np.ascontiguousarray(d["org"], F)
        self.n = n = len(self.prim)
        self.rays = np.zeros((n, 8), F)
        self.rays[:, 0:3], self.rays[:, 4:7], self.rays[:, 7] = self.org, (0.0, 0.0, -1.0), 1e38
        self.hits = np.zeros((n, 4), F)
        self.hits[:, 0], self.hits[:, 1:3] = 1.0, self.uv
        self.hits.view(np.int32)[:, 3] = self.prim


def _views(rng, sc, prim, uv, below=0.25):
    """ordinary origins: 0.5 to 2 above the hit (or below, for a share of the rows), off to the side"""
    n = len(prim)
    with np.errstate(all="ignore"):
        p = np.nan_to_num(sc.pos32(prim, uv[:, 0], uv[:, 1]), nan=0.0, posinf=1e30, neginf=-1e30)
    side = np.where(rng.uniform(size=n) < below, -1.0, 1.0)
    off = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), side * rng.uniform(0.5, 2.0, n)], axis=1)
    return (p + off).astype(F)


def _ordinary(rng, sc, n, quads=None):
    quads = sc.ordinary_quads if quads is None else np.asarray(quads)
    q = quads[rng.integers(0, len(quads), n)]
    prim = (2 * q + np.where(np.isin(q, sc.a_only), 0, rng.integers(0, 2, n))).astype(np.int32)
    a, b = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    fold = a + b > 1
    uv = np.stack([np.where(fold, 1 - a, a), np.where(fold, 1 - b, b)], axis=1).astype(F)
    return dict(prim=prim, uv=uv, org=_views(rng, sc, prim, uv))


def _on_a(rng, sc, quad, uv):
    """records on triangle A of the given quads (there the texture coordinate is the barycentric pair)"""
    prim = (2 * np.asarray(quad)).astype(np.int32)
    uv = np.ascontiguousarray(uv, F)
    return dict(prim=prim, uv=uv, org=_views(rng, sc, prim, uv))


def _addressing(rng, sc, n, gen):
    """records over the nine addressing quads: record i is on shape i % 9, gen(j, w, h) -> (u, v) for its j-th record"""
    quad, uv = [], []
    for i in range(n):
        s = i % len(SHAPES)
        quad.append(sc.quads[("addr", s)])
        uv.append(gen(i // len(SHAPES), *SHAPES[s]))
    return _on_a(rng, sc, quad, np.array(uv, F))


INT_RANGE_TARGETS = (2.0 ** 31 - 128, 2.0 ** 31, 2.0 ** 31 + 256, 1e12, 3e38, np.inf, np.nan)


def texcoord_for(t, sgn, side):
    """a coordinate whose fp32 u * side - 0.5 is sgn * t (NaN, inf and 3e38 themselves; the nearest product otherwise)"""
    if np.isnan(t):
        return F(np.nan)
    if np.isinf(t):
        return F(sgn * np.inf)
    if t == 3e38:
        return F(sgn * 3e38)  # u * side overflows to inf for side >= 2 and stays 3e38 for side 1
    u0 = F(sgn * t / side)
    for s_ in range(-3, 4):  # the step whose product is the target itself, where there is one
        if texel32(step(u0, s_)[()], side)[0] == F(sgn * t):
            return step(u0, s_)[()]
    return u0


def families(sc, seed=1, n=FAMILY_N):
    """name -> dict(prim, uv, org) of n records on EdgeScene sc"""
    rng = np.random.default_rng(seed)
    fam = {"ordinary": _ordinary(rng, sc, n)}
    inside = lambda: float(rng.uniform(0.05, 0.95))  # noqa: E731

    def centres(j, w, h):
        tx, ty = j % (w + 2) - 1, (3 * j + j // (w + 2)) % (h + 2) - 1
        if w == 100:
            tx, ty = (37 * j) % (w + 2) - 1, (11 * j) % (h + 2) - 1
        while True:
            u, v = _solve(tx, w), _solve(ty, h)
            if u is not None and v is not None:
                return u, v
            tx, ty = tx + (u is None), ty + (v is None)
    fam["texel_centres"] = _addressing(rng, sc, n, centres)

    def edges(j, w, h):
        tx, ty = j % (w + 1) - 1, (j // 3) % (h + 1) - 1
        u, v = _solve(tx, w, 0.5), _solve(ty, h, 0.5)
        u = F(inside()) if u is None else step(u, (j % 3) - 1)[()]
        v = F(inside()) if v is None else step(v, ((j // 3) % 3) - 1)[()]
        return (u, v) if j % 2 == 0 or w == 1 else (u, F(inside()))
    fam["texel_edges"] = _addressing(rng, sc, n, edges)

    seam = [step(F(b), k)[()] if b != 0 or k == 0 else F(TINY * k) for b in (0.0, 1.0, -1.0, 2.0) for k in (-1, 0, 1)]
    fam["seams"] = _addressing(rng, sc, n, lambda j, w, h: (seam[j % 12], seam[(5 * j + j // 12) % 12]))

    def last(j, w, h):
        e = ((w - 0.5) / w, (w + 0.5) / w), ((h - 0.5) / h, (h + 0.5) / h)
        pick = lambda lo, hi, k: F(lo) if k == 0 else step(F(hi), -1)[()] if k == 1 else F(rng.uniform(lo, hi))  # noqa: E731
        return pick(*e[0], j % 4), pick(*e[1], (j // 4) % 4)
    fam["last_texel"] = _addressing(rng, sc, n, last)

    # triangle B of the addressing quads: UV = (2^24 u, -2^24 v)
    def on_b(gen):
        d = _addressing(rng, sc, n, lambda j, w, h: tuple(F(abs(c) / UV_SCALE) for c in gen(j, w, h)))
        d["prim"] = d["prim"] + 1
        d["org"] = _views(rng, sc, d["prim"], d["uv"])
        return d
    mags = (3.7, 1e4, 1e7)
    fam["far"] = on_b(lambda j, w, h: (mags[j % 3] * rng.uniform(0.9, 1.1), mags[(j // 3) % 3] * rng.uniform(0.9, 1.1)))
    fam["fraction_lost"] = on_b(lambda j, w, h: (2.0 ** rng.uniform(23, 25) / w, 2.0 ** rng.uniform(23, 25) / h if j % 2 else 3.7 * inside()))

    signed = [(t, sgn) for t in INT_RANGE_TARGETS for sgn in (1, -1)]
    count = [0]

    def int_range(j, w, h):
        def coord(k, side):
            t, sgn = signed[k % len(signed)]
            return texcoord_for(3e38 if np.isinf(t) else t, sgn, side)
        c = count[0]
        count[0] += 1
        ku, kv = c // 3, 5 * (c // 3) + 2
        return (coord(ku, w), F(inside())) if c % 3 == 0 else (F(inside()), coord(kv, h)) if c % 3 == 1 else (coord(ku, w), coord(kv, h))
    fam["int_range"] = _addressing(rng, sc, n, int_range)

    rng = np.random.default_rng((seed, 1))
    # -- texcoords on the edges of the int range, hit at their corner (b = 1, 0, 0: the vertex's own texcoord, exactly)
    k = np.arange(n)
    corners = np.array([(0, 0), (1, 0), (0, 1)], F)
    prim = np.array(sc.range_tris, np.int32)[k % len(sc.range_tris)]
    uv = corners[(k // len(sc.range_tris)) % 3]
    fam["texcoord_range"] = dict(prim=prim, uv=uv, org=_views(rng, sc, prim, uv))

    # -- barycentrics
    k = np.arange(n)
    one_up = step(F(0.75), 1)[()]
    special = np.array([(0, 0), (1, 0), (0, 1), (0.5, 0), (0, 0.5), (0.5, 0.5), (0.25, 0.75), (one_up, 0.25), (0.25, one_up),
                        (1.5, -0.25), (-0.25, 1.5), (-0.0, -0.0), (np.nan, 0.25), (0.25, np.nan), (np.inf, 0.25), (0.25, -np.inf)], F)
    uv = special[k % len(special)]
    q = np.array(sc.quad_list("addr") + [sc.quads["plain_ds"], sc.quads["plain_ss"]])[k // len(special) % 11]
    prim = (2 * q + np.where(np.isin(q, sc.a_only), 0, (k // 7) % 2)).astype(np.int32)
    fam["bary"] = dict(prim=prim, uv=uv, org=_views(rng, sc, prim, uv))

    rng = np.random.default_rng((seed, 2))
    # -- vertex normals
    nq = np.array(sc.quad_list("normals"))
    d = _ordinary(rng, sc, n, nq)
    if ("normals", "opposite") in sc.quads:  # the edge midpoints where the sum is exactly zero
        ko = sc.quads[("normals", "opposite")]
        m = (d["prim"] // 2 == ko) & (k % 2 == 0)
        d["prim"][m] = 2 * ko
        d["uv"][m] = (0.5, 0.0)  # v0 and v1 are opposite
    fam["normals"] = d

    rng = np.random.default_rng((seed, 3))
    # -- origins: every other row on an edge, the rest ordinary (above, and below: behind a single- and a double-sided surface)
    d = _ordinary(rng, sc, n, [sc.quads["plain_ds"], sc.quads["plain_ss"]])
    p = sc.pos32(d["prim"], d["uv"][:, 0], d["uv"][:, 1])
    kind = np.where(k % 2 == 0, (k // 2) % 8, -1)
    o = d["org"]
    o[kind == 0] = p[kind == 0]                                          # at posW: V is NaN
    for kk, z in ((1, 0.0), (2, float(TINY)), (3, -float(TINY))):        # in the tangent plane (N.V == 0), a step either side
        o[kind == kk, 2] = z
    o[kind == 4, 2] = -np.abs(o[kind == 4, 2])                           # behind
    with np.errstate(all="ignore"):
        away = (o - p) / np.linalg.norm(o - p, axis=1, keepdims=True)
    o[kind == 5] = (p + away * 1e-20)[kind == 5]                          # 1e-20 away (rounds to posW where posW is not 0)
    o[kind == 6] = (away * 1e20)[kind == 6]                               # 1e20 away: the squared distance overflows
    o[kind == 7, 2] = np.where(k[kind == 7] % 4 == 0, 1e-3, -1e-3)       # close to the tangent plane, but clear of it
    fam["origin"] = dict(d, org=o.astype(F))

    fam["decode"] = _ordinary(rng, sc, n, sc.quad_list("decode"))

    rng = np.random.default_rng((seed, 4))
    # -- normal map: texel centres of the eight map texels, the midpoint of 127 | 128, and ordinary hits
    nmq = np.array(sc.quad_list("nmap"))
    q = nmq[k % len(nmq)]
    cen = ((k // len(nmq)) % 8 + 0.5) / 8
    u = np.where(k % 5 == 0, 0.5, np.where(k % 5 == 1, rng.uniform(0, 1, n), cen))  # 0.5: x = 3.5, half of 127 and half of 128
    fam["normal_map"] = _on_a(rng, sc, q, np.stack([u, rng.uniform(0.05, 0.9, n) * (1 - np.minimum(u, 1))], axis=1))

    rng = np.random.default_rng((seed, 5))
    # -- alpha
    # every ill-conditioned family: every other row sits on its tie, the rest well clear of one
    cards = lambda lst, clear: np.where(k % 2 == 0, np.array(lst)[(k // 2) % len(lst)], np.array(clear)[(k // 2) % len(clear)])  # noqa: E731
    rnd_uv = np.stack([rng.uniform(-1.5, 2.5, n), rng.uniform(-1.5, 2.5, n)], axis=1)
    fam["tie_const"] = _on_a(rng, sc, cards(sc.const_cards, sc.clear_cards), rnd_uv)
    fam["tie_flat_texture"] = _on_a(rng, sc, cards(sc.flat_cards, sc.clear_cards + sc.quad_list("addr")), rnd_uv[::-1])
    # fx (2 x 1) or fy (1 x 2) exactly 0.5 at uv 0.5 (x = 0.5: bytes 0 and 255) and 1.0 (x = 1.5: 255 and 0), a step either side
    half = np.where(k // 2 % 2 == 0, F(0.5), F(1.0))
    near = np.array([step(h_, (i // 4) % 3 - 1)[()] for i, h_ in enumerate(half)], F)
    clear = np.where(k // 2 % 2 == 0, F(0.25), F(0.75)) + (k // 4 % 4) * F(0.03125)
    t = np.where(k % 2 == 0, near, clear).astype(F)
    q = np.array(sc.bilinear_cards)[(k // 16) % 2]
    other = rng.uniform(0.1, 0.9, n).astype(F)
    is_w = q == sc.bilinear_cards[0]
    fam["tie_bilinear"] = _on_a(rng, sc, q, np.stack([np.where(is_w, t, other), np.where(is_w, other, t)], axis=1))
    fam["unused"] = _on_a(rng, sc, cards(sc.unused_cards, sc.clear_cards), rnd_uv)
    uv = np.where((k % 2 == 0)[:, None], np.stack([rng.uniform(0.3, 0.7, n), rng.uniform(0.3, 0.7, n)], axis=1), 0.0)  # alpha 0 there, 1 at (0, 0)
    fam["types_3_to_7"] = _on_a(rng, sc, np.array(sc.type_cards)[(k // 2) % 5], uv)
    for v in fam.values():
        assert len(v["prim"]) == n and v["uv"].shape == (n, 2) and v["org"].shape == (n, 3)
    return fam


ALPHA_FAMILIES = ("tie_const", "tie_flat_texture", "tie_bilinear", "unused", "types_3_to_7")
ADDRESS_FAMILIES = ("texel_centres", "texel_edges", "seams", "last_texel", "far", "fraction_lost", "int_range", "texcoord_range")
# ill-conditioned: compared by class outside the margin
ILL = ("bary", "normals", "origin", "normal_map", "int_range") + ALPHA_FAMILIES


def records(sc, name, seed=1):
    d = families(sc, seed)[name]
    return SurfaceRecords(d, np.zeros(len(d["prim"]), np.int32), [name])


def mixed(sc, seed=1):
    """every family and as many ordinary records again, interleaved in one fixed random order"""
    fam = families(sc, seed)
    rng = np.random.default_rng(seed + 1000)
    fam["random"] = _ordinary(rng, sc, sum(len(v["prim"]) for v in fam.values()))
    d, label, names = _interleave(fam, rng)
    return SurfaceRecords(d, label, names)


def down_rays(sc, seed=1, per_quad=32):
    """rays straight down from z = 1 onto dyadic points (multiples of 1/16) of every quad, in the layout of oracle_trace
    (org, dir, tmin, tmax): exact barycentrics on either triangle"""
    rng = np.random.default_rng(seed + 2000)
    q = np.repeat(np.arange(sc.nq - ("ceiling" in sc.quads)), per_quad)
    x = rng.integers(0, 17, len(q)) / 16.0
    y = rng.integers(0, 17, len(q)) / 16.0
    corner = np.array([t // 2 for t in sc.range_tris for _ in range(4)], np.int64)  # the corner only triangle B has: its texcoord, exactly
    q, x, y = np.concatenate([q, corner]), np.concatenate([x, np.ones(len(corner))]), np.concatenate([y, np.ones(len(corner))])
    r = np.zeros((len(q), 8), F)
    r[:, 0], r[:, 1], r[:, 2] = 2 * q + x, y, 1.0
    r[:, 5], r[:, 6], r[:, 7] = -1.0, 0.0, 1e38
    r[1::4, 2], r[1::4, 5] = -1.0, 1.0  # every fourth from below
    return r
