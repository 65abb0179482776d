"""Edge-case shading records for the BSDF, light and connection tests (tests/test_shading_edge_records_cpu.py,
tests/test_gpu_shading_edge_records.py): named families of records no frame produces.  Seeded, plain numpy; no product
code.  Only float fields take extreme values: prim and material stay valid (or prim is -1, the documented miss), light
indices, counts and buffer sizes stay inside each call's contract.

  bsdf_families / bsdf_mixed         the 20-float records of bdpt_test_bsdf with the matching bdpt_surface records, seeds
                                     and dirs of bdpt_bsdf_query (the roughness of the former is the fp32 square of the
                                     linearRoughness of the latter, as the query forms it)
  light_cases                        light sets of 1, 3 and 4 lights with the NEE records of bdpt_light_query
  vertex_families / vertex_mixed     eye / light pairs of BDPT_CONNECT_VERTICES
  camera_families / camera_mixed     light vertices of BDPT_CONNECT_CAMERA for one camera, frame and jitter

A family's name says which edge it sits on; the CPU test's docstrings say why a family is ill-conditioned.

Measured on the CPU, the oracle (fp32, fixed polynomial transcendentals) against the float64 reading
(tests/hlsl_reference_math.py, tests/hlsl_light_connect_math.py), 2026-10-19, FAMILY_N = 256 records per family, worst
error over the rows the margin rule (1e-6) keeps; rel = relative over a floor of 1e-4, dir = absolute.  Bound: the
project's 5e-4 (rel) and 1e-4 (dir) for every call; no call needed another (ordinary light, vertex and camera records:
6.7e-6, 1.3e-5, 1.2e-5).  "class" = ill-conditioned: only the branch and the finite / zero / non-finite class of every
output word are compared.  `python tests/test_shading_edge_records_cpu.py` prints the table per matIndex.

  family (worst over matIndex; camera: four frames) rows  left out   worst error, or "class"
  bsdf/ordinary                              256         0   rel 4.1e-05  dir 1.2e-05
  bsdf/rough_one                             256         0   rel 1.1e-05  dir 5.6e-07
  bsdf/v_l_n_equal                           256         0   rel 9.5e-06  dir 2.3e-05
  bsdf/l_is_minus_v                          256         0   rel 1.0e-04  dir 5.6e-05
  bsdf/black                                 256         0   rel 7.9e-05  dir 1.5e-05
  bsdf/white                                 256         0   rel 6.6e-05  dir 8.2e-06
  bsdf/subnormal_colours                     256         0   rel 5.5e-05  dir 1.7e-05
  bsdf/nonunit_n                             256         0   rel 4.1e-06  dir 1.4e-05
  bsdf/first_draw_zero                       256         0   rel 2.0e-06  dir 1.1e-07
  bsdf/axis_normals                          256         0   rel 8.6e-06  dir 6.6e-06
  bsdf/v_below                               256         0   rel 2.3e-05  dir 3.3e-06
  bsdf/spec_one                              256         0   rel 2.4e-04  dir 1.9e-05
  bsdf/ggx_d_clamp                           256         0   rel 2.6e-05  dir 1.2e-05
  bsdf/ndoth_one                             256         0   rel 2.5e-05  dir 1.0e-05
  bsdf/luminance_clamp                       256         0   rel 6.7e-05  dir 8.0e-06
  bsdf/nonfinite_colour                      256         0   rel 1.9e-05  dir 1.6e-05
  bsdf/rough_to_zero                         256        74   class
  bsdf/v_tangent                             256         0   class
  bsdf/l_tangent                             256         0   class
  bsdf/lobe_tie                              256       256   class
  bsdf/draw_edges                            256         0   class
  light/one_point/ordinary_point             256         0   rel 6.7e-06  dir 1.2e-07
  light/one_point/dist2_threshold            256       224   class
  light/one_point/dist2_overflow             256       256   class
  light/one_point/nl_zero                    256         0   class
  light/one_point/back_facing                256         0   rel 8.8e-08  dir 1.2e-07
  light/one_point/v_is_minus_l               256         0   rel 2.6e-06  dir 1.2e-07
  light/one_point/miss                       256         0   rel 0.0e+00  dir 0.0e+00
  light/one_point_tiny/dist2_underflow       256         0   rel 1.0e-26  dir 0.0e+00
  light/cone_edge/cone_edge                  256       256   class
  light/cone_edge/cone_inside_outside        256         0   rel 3.0e-06  dir 1.2e-07
  light/penumbra/penumbra                    256         1   rel 2.3e-06  dir 1.1e-07
  light/opening_and_dir/opening_and_dir      256        96   class
  light/directional/directional              256         0   rel 3.5e-06  dir 5.2e-08
  light/intensity/intensity                  256         0   rel 4.4e-06  dir 1.1e-07
  light/selection_3/selection                256       139   class
  light/selection_4/selection                256       164   class
  vertices/ordinary                          256         0   rel 1.3e-05  dir 1.0e-07
  vertices/coincident                        256         0   class
  vertices/one_step_apart                    256         0   class
  vertices/apart_1e-20                       256       256   class
  vertices/apart_1e15                        256         0   rel 6.0e-08  dir 7.1e-08
  vertices/apart_1e20                        256       256   class
  vertices/tangent_planes                    256         0   class
  vertices/connectdir_is_wol                 256         0   class
  vertices/prev_is_vertex                    256         0   class
  vertices/black                             256         0   rel 1.2e-05  dir 1.0e-07
  vertices/fsl_zero                          256         0   class
  vertices/fse_zero                          256         0   class
  vertices/spec_flags                        256         0   rel 1.2e-05  dir 9.4e-08
  vertices/miss                              256         0   rel 1.1e-05  dir 8.0e-08
  camera/ordinary                           1024         0   rel 1.2e-05  dir 1.1e-07
  camera/edge_x                             1024       412   class
  camera/edge_y                             1024       424   class
  camera/corner                             1024       659   class
  camera/tie_x                              1024      1024   class
  camera/tie_y                              1024      1024   class
  camera/camera_plane                       1024      1024   class
  camera/behind                             1024         0   rel 8.8e-08  dir 1.4e-07
  camera/at_camera                          1024       512   class
  camera/far_1e20                           1024      1024   class
  camera/v_is_minus_dir                     1024         0   class
  camera/miss                               1024         0   rel 0.0e+00  dir 0.0e+00

A family that is all "left out" sits wholly inside a margin by construction (ties, thresholds, fp32 over- and underflow):
there the CPU test asserts that the family reaches its edge, and the GPU test compares kernel and oracle bit for bit.
"""
import ctypes as C

import numpy as np

F = np.float32
FAMILY_N = 256
LCG_A, LCG_C = 1664525, 1013904223
LCG_INV = pow(LCG_A, -1, 2 ** 32)
TOP24 = 0x00FFFFFF
PI32 = F(3.14159265358979323846)


# ---- fp32 helpers in the operation order of device_math.hpp ----------------------------------------------------------
def dot3(a, b):
    with np.errstate(all="ignore"):
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize3(a):
    with np.errstate(all="ignore"):
        inv = F(1.0) / np.sqrt(dot3(a, a))
        return (a * inv[..., None]).astype(F)


def step(x, k):
    """x moved k fp32 steps (k of either sign) toward +-inf"""
    x = np.asarray(x, F).copy()
    for _ in range(abs(int(k))):
        x = np.nextafter(x, F(np.inf if k > 0 else -np.inf))
    return x


def lcg(s):
    s1 = ((np.asarray(s).astype(np.uint64) * LCG_A + LCG_C) & 0xFFFFFFFF).astype(np.uint32)
    return s1, ((s1 & TOP24).astype(F) / F(16777216.0)).astype(F)


def lcg_back(s1, steps=1):
    s = np.asarray(s1).astype(np.uint64)
    for _ in range(steps):
        s = ((s - LCG_C) * LCG_INV) & 0xFFFFFFFF
    return s.astype(np.uint32)


def seeds_with_draw(rng, low24, draw=1):
    """states whose draw-th nextRand has the low 24 bits `low24` (an array): the float low24 / 2^24"""
    low24 = np.asarray(low24, np.uint64)
    hi = rng.integers(0, 256, len(low24)).astype(np.uint64) << 24
    return lcg_back((hi | low24).astype(np.uint32), draw)


def unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


class Batch:
    """records of several families: label per row and the families' names"""

    def __init__(self, family, names):
        self.family, self.names = family, names

    def of(self, name):
        return self.family == self.names.index(name)

    def tally(self, bad):
        """rows per family where `bad`, for an assertion's message"""
        return {n: int(bad[self.family == i].sum()) for i, n in enumerate(self.names) if bad[self.family == i].any()}


def _interleave(parts, rng):
    """parts: name -> dict of equally long arrays.  -> (dict of concatenated arrays in one fixed random order, labels, names)"""
    names = list(parts)
    keys = list(parts[names[0]])
    n_of = [len(parts[k][keys[0]]) for k in names]
    label = np.concatenate([np.full(m, i, np.int32) for i, m in enumerate(n_of)])
    order = rng.permutation(len(label))
    out = {k: np.ascontiguousarray(np.concatenate([parts[nm][k] for nm in names])[order]) for k in keys}
    return out, label[order], names


# ---- BSDF records ----------------------------------------------------------------------------------------------------
def _ordinary(rng, n):
    """the records of test_bsdf_parity: unit vectors, V mostly above the surface, linearRoughness in [0.08, 1)"""
    Nn, V, L = unit(rng, n), unit(rng, n), unit(rng, n)
    V = np.where((np.sum(Nn * V, axis=1, keepdims=True) < 0) & (rng.uniform(size=(n, 1)) < 0.9), -V, V).astype(F)
    return dict(N=Nn, V=V, L=L, dif=rng.uniform(0, 1, (n, 3)).astype(F), spec=rng.uniform(0, 1, (n, 3)).astype(F),
                lr=rng.uniform(0.08, 1, n).astype(F), is_spec=rng.integers(0, 2, n).astype(F),
                seed=rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32), prim=rng.integers(0, 1000, n).astype(np.int32))


def _tangent_pair(rng, n):
    """(N, T): unit vectors (to fp32 rounding) whose fp32 dot product is exactly 0: T = (c, -s, 0), N = (s/2, c/2, sqrt(3)/2)"""
    a = rng.uniform(0, 2 * np.pi, n)
    s, c = np.sin(a).astype(F), np.cos(a).astype(F)
    T = np.stack([c, -s, np.zeros(n, F)], axis=1).astype(F)
    Nn = np.stack([F(0.5) * s, F(0.5) * c, np.full(n, np.sqrt(0.75), F)], axis=1).astype(F)
    assert (dot3(Nn, T) == 0).all()
    return Nn, T


def _signed_zero_axes():
    out = []
    for k in range(3):
        for s in (1.0, -1.0):
            for za in (0.0, -0.0):
                for zb in (0.0, -0.0):
                    d = [za, zb]
                    d.insert(k, s)
                    out.append(d)
    return np.array(out, F)


def _prob_diffuse32(dif, spec):
    """probabilityToSampleDiffuse in fp32 (finite colours)"""
    w = np.array([0.2126, 0.7152, 0.0722], F)
    ld = np.maximum(F(0.01), dot3(dif, w[None]))
    ls = np.maximum(F(0.01), dot3(spec, w[None]))
    return (ld / (ld + ls)).astype(F)


ROUGH_TO_ZERO_LR = np.array([0.0, 1e-30, 1e-15, 1e-10, 1e-4, 1e-2, 0.0316227766], F)  # roughness 0, 0 (underflow), 1e-30, 1e-20, 1e-8, 1e-4, 1e-3


def bsdf_families(seed=1, n=FAMILY_N):
    rng = np.random.default_rng(seed)
    fam = {}

    def new(name):
        fam[name] = _ordinary(rng, n)
        return fam[name]

    new("ordinary")
    new("rough_one")["lr"][:] = 1.0
    d = new("rough_to_zero")
    d["lr"][:] = ROUGH_TO_ZERO_LR[np.arange(n) % len(ROUGH_TO_ZERO_LR)]
    d = new("v_tangent")
    d["N"], d["V"] = _tangent_pair(rng, n)
    d = new("l_tangent")
    d["N"], d["L"] = _tangent_pair(rng, n)
    d["V"] = np.where(dot3(d["N"], d["V"])[:, None] < 0, -d["V"], d["V"]).astype(F)
    d = new("l_is_minus_v")
    d["L"] = np.negative(d["V"])
    d = new("v_l_n_equal")
    d["V"] = d["N"].copy()
    d["L"] = d["N"].copy()
    d = new("v_below")
    d["V"] = np.where(dot3(d["N"], d["V"])[:, None] > 0, -d["V"], d["V"]).astype(F)
    d = new("axis_normals")
    ax = _signed_zero_axes()
    d["N"] = ax[np.arange(n) % len(ax)].copy()
    d = new("nonunit_n")
    d["N"] = (d["N"] * np.array([0.5, 2.0, 1e-3], F)[np.arange(n) % 3][:, None]).astype(F)
    d = new("subnormal_colours")
    d["dif"][:] = np.where(np.arange(n)[:, None] % 2 == 0, F(1e-40), F(1e-41))
    d["spec"][:] = np.where(np.arange(n)[:, None] % 4 < 2, F(1e-41), F(1e-40))
    d = new("black")
    d["dif"][:] = 0.0
    d["spec"][:] = 0.0
    d = new("white")  # spec == 1: the Fresnel term is exactly 1 whatever L.H
    d["dif"][:] = 1.0
    d["spec"][:] = 1.0
    d = new("spec_one")
    d["spec"][:] = 1.0
    d = new("first_draw_zero")
    d["seed"] = seeds_with_draw(rng, np.zeros(n, np.uint64), 1)
    # d * d * pi of ggxNormalDistribution on either side of its 0.001 clamp: V and L mirrored about H in the plane of N and H,
    # N.H^2 (1 - a2) = 1 - sqrt(0.001 / pi) up to a few steps either way
    d = new("ggx_d_clamp")
    d["lr"][:] = np.sqrt(0.05)
    a2 = 0.05 ** 2  # roughness = linearRoughness^2 = 0.05
    ndoth = np.sqrt((1.0 - np.sqrt(0.001 / np.pi)) / (1.0 - a2)) * (1.0 + rng.uniform(-4e-6, 4e-6, n))
    th, ph = np.arccos(ndoth), rng.uniform(0.1, 0.6, n)
    d["N"] = np.tile(np.array([[0, 0, 1]], F), (n, 1))
    d["V"] = np.stack([np.sin(th + ph), np.zeros(n), np.cos(th + ph)], axis=1).astype(F)
    d["L"] = np.stack([np.sin(th - ph), np.zeros(n), np.cos(th - ph)], axis=1).astype(F)
    d["is_spec"][:] = 1.0
    # N.H == 1: V and L mirrored about N
    d = new("ndoth_one")
    th = rng.uniform(0.05, 1.5, n)
    d["N"] = np.tile(np.array([[0, 0, 1]], F), (n, 1))
    d["V"] = np.stack([np.sin(th), np.zeros(n), np.cos(th)], axis=1).astype(F)
    d["L"] = d["V"] * np.array([[-1, 1, 1]], F)
    d["is_spec"][:] = 1.0
    # luminance of dif and of spec on either side of the 0.01 clamp of probabilityToSampleDiffuse
    d = new("luminance_clamp")
    g = step(np.full(n, 0.01, F), 0)
    for k in range(n):
        g[k] = step(g[k], (k % 9) - 4)
    d["dif"] = np.repeat(g[:, None], 3, axis=1)
    d["spec"] = np.repeat(g[::-1, None], 3, axis=1).copy()
    d = new("nonfinite_colour")
    bad = np.array([np.inf, np.nan, -np.inf], F)
    for k in range(n):
        d["dif" if (k // 9) % 2 == 0 else "spec"][k, k % 3] = bad[(k // 3) % 3]
    # draws of exactly 0 and of 1 - 2^-24, for each of the three draws of sampleBRDF (lobe choice, r0, r1)
    d = new("draw_edges")
    k = np.arange(n)
    low = np.where(k % 2 == 0, 0, TOP24).astype(np.uint64)
    for draw in (1, 2, 3):
        m = (k // 2) % 3 == draw - 1
        d["seed"][m] = seeds_with_draw(rng, low[m], draw)
    # the lobe choice within one fp32 step of its boundary: grey colours whose probDiffuse is the first draw, or one step off
    d = new("lobe_tie")
    d["seed"] = seeds_with_draw(rng, rng.integers(int(0.2 * 2 ** 24), int(0.8 * 2 ** 24), n).astype(np.uint64), 1)
    _, r = lcg(d["seed"])
    ls = F(0.5)
    ld0 = (r.astype(np.float64) * 0.5 / (1.0 - r.astype(np.float64))).astype(F)
    best, best_gap = ld0.copy(), np.full(n, np.inf)
    want = step(r, 0)
    for i in range(n):
        want[i] = step(r[i], (i % 3) - 1)  # probDiffuse one step below, at, one step above the draw
    for k in range(-6, 7):
        cand = step(ld0, k)
        pd = _prob_diffuse32(np.repeat(cand[:, None], 3, axis=1), np.full((n, 3), ls, F))
        gap = np.abs(pd.astype(np.float64) - want.astype(np.float64))
        better = gap < best_gap
        best[better], best_gap[better] = cand[better], gap[better]
    d["dif"] = np.repeat(best[:, None], 3, axis=1)
    d["spec"] = np.full((n, 3), ls, F)
    # the documented miss, with every float field extreme
    d = new("miss")
    d["prim"][:] = -1
    d["N"][::2] = np.nan
    d["dif"][1::2] = np.inf
    return fam


BSDF_FIRST_GROUP = ("ordinary", "rough_one", "v_l_n_equal", "l_is_minus_v", "black", "white", "subnormal_colours", "nonunit_n",
                    "first_draw_zero", "axis_normals", "v_below")


class BsdfRecords(Batch):
    def __init__(self, d, family, names):
        super().__init__(family, names)
        n = len(d["lr"])
        self.n, self.seeds, self.prim = n, np.ascontiguousarray(d["seed"], np.uint32), np.ascontiguousarray(d["prim"], np.int32)
        self.rec = np.zeros((n, 20), F)
        self.rec[:, 0:3], self.rec[:, 3:6], self.rec[:, 6:9] = d["N"], d["V"], d["L"]
        self.rec[:, 9:12], self.rec[:, 12:15] = d["dif"], d["spec"]
        with np.errstate(all="ignore"):
            self.rec[:, 15] = d["lr"] * d["lr"]  # fp32, as the query squares linearRoughness
        self.rec[:, 16] = d["is_spec"]
        self.rec[:, 17] = self.seeds.view(F)
        self.surf = np.zeros((n, 24), F)
        self.surf[:, 4:7], self.surf[:, 7], self.surf[:, 8:11] = d["N"], d["lr"], d["V"]
        self.surf[:, 12:15], self.surf[:, 16:19] = d["dif"], d["spec"]
        self.surf.view(np.int32)[:, 23] = self.prim
        self.dirs = np.ascontiguousarray(np.concatenate([d["L"], d["is_spec"][:, None]], axis=1), F)


def bsdf_records(name, seed=1):
    d = bsdf_families(seed)[name]
    return BsdfRecords(d, np.zeros(len(d["lr"]), np.int32), [name])


def bsdf_mixed(seed=1):
    """every family and as many ordinary records again, interleaved in one fixed random order"""
    fam = bsdf_families(seed)
    rng = np.random.default_rng(seed + 1000)
    fam["random"] = _ordinary(rng, sum(len(v["lr"]) for v in fam.values()))
    d, label, names = _interleave(fam, rng)
    return BsdfRecords(d, label, names)


# ---- light records ---------------------------------------------------------------------------------------------------
LIGHT_POINT, LIGHT_DIRECTIONAL = 0, 1


def light(kind=LIGHT_POINT, pos=(0.25, 0.5, 2.0), direction=(0.0, 0.0, -1.0), opening=np.pi, penumbra=0.0, intensity=(3.0, 2.0, 1.0),
          cos_opening=None):
    """a bdpt_light as a dict of plain numbers (make_lights turns it into the ctypes record)"""
    return dict(type=kind, posW=tuple(float(F(x)) for x in pos), dirW=tuple(float(F(x)) for x in direction), openingAngle=float(F(opening)),
                penumbraAngle=float(F(penumbra)), intensity=tuple(float(F(x)) for x in intensity),
                cosOpeningAngle=float(F(np.cos(np.float64(F(opening))))) if cos_opening is None else float(F(cos_opening)))


def make_lights(abi, lights):
    arr = (abi.Light * len(lights))()
    for i, l in enumerate(lights):
        arr[i].type = l["type"]
        for k in range(3):
            arr[i].posW[k], arr[i].dirW[k], arr[i].intensity[k] = l["posW"][k], l["dirW"][k], l["intensity"][k]
        arr[i].openingAngle, arr[i].penumbraAngle, arr[i].cosOpeningAngle = l["openingAngle"], l["penumbraAngle"], l["cosOpeningAngle"]
    return arr


def seeds_for_light(rng, which, count):
    """states whose selection draw picks light which[i] of count"""
    which = np.asarray(which)
    lo = np.ceil(which * (2 ** 24) / count).astype(np.int64)
    hi = np.ceil((which + 1) * (2 ** 24) / count).astype(np.int64)
    low24 = rng.integers(lo, hi)
    s = seeds_with_draw(rng, low24.astype(np.uint64), 1)
    _, r = lcg(s)
    assert np.array_equal(np.minimum((r * F(count)).astype(np.int32), count - 1), which)
    return s


def _surface_at(rng, pos, n_toward=None):
    """ordinary shading fields at the given positions; N within the hemisphere of n_toward (so that the light is in front)"""
    n = len(pos)
    d = _ordinary(rng, n)
    s = np.zeros((n, 24), F)
    Nn = d["N"]
    if n_toward is not None:
        with np.errstate(all="ignore"):
            flip = np.nan_to_num(dot3(Nn, n_toward.astype(F))) < 0
        Nn = np.where(flip[:, None], -Nn, Nn).astype(F)
    V = np.where(dot3(Nn, d["V"])[:, None] < 0, -d["V"], d["V"]).astype(F)
    s[:, 0:3], s[:, 4:7], s[:, 7], s[:, 8:11], s[:, 12:15], s[:, 16:19] = pos, Nn, d["lr"], V, d["dif"], d["spec"]
    s.view(np.int32)[:, 23] = d["prim"]
    return s


class LightCase(Batch):
    """one light set (1, 3 or 4 lights) and its NEE records; `which` is the light each record's seed selects"""

    def __init__(self, name, lights, surf, seeds, which, family, names, ill):
        super().__init__(family, names)
        self.name, self.lights, self.surf, self.seeds, self.which, self.ill = name, lights, np.ascontiguousarray(surf, F), seeds, which, ill
        self.n = len(seeds)


def _case(name, lights, parts, rng, ill):
    """parts: family name -> (surf, which).  Seeds select `which`; the families are interleaved."""
    count = len(lights)
    fam = {k: dict(surf=s, which=np.asarray(w, np.int64), seed=seeds_for_light(rng, np.asarray(w, np.int64), count)) for k, (s, w) in parts.items()}
    d, label, names = _interleave(fam, rng)
    return LightCase(name, lights, d["surf"], np.ascontiguousarray(d["seed"], np.uint32), d["which"], label, names, ill)


def _around(rng, lights, which, n, lo=0.5, hi=3.0):
    """positions at ordinary distances from the selected lights, N toward the light"""
    lp = np.array([lights[w]["posW"] for w in which], F)
    off = unit(rng, n) * rng.uniform(lo, hi, (n, 1)).astype(F)
    pos = (lp + off).astype(F)
    return _surface_at(rng, pos, (lp - pos))


def _in_cone(rng, lights, which, n, spread):
    """positions below the selected lights (dirW = -z) at polar angles up to `spread`"""
    lp = np.array([lights[w]["posW"] for w in which], F)
    th, ph, dist = rng.uniform(0, spread, n), rng.uniform(0, 2 * np.pi, n), rng.uniform(0.5, 3.0, n)
    off = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), -np.cos(th)], axis=1) * dist[:, None]
    pos = (lp + off.astype(F)).astype(F)
    return _surface_at(rng, pos, (lp - pos))


def light_cases(seed=1, n=FAMILY_N):
    """-> list of LightCase.  `ill` names the families of a case that sit on a branch (class comparison only)."""
    rng = np.random.default_rng(seed + 2000)
    cases = []
    cyc = lambda k, m=n: np.arange(m) % k  # noqa: E731

    # -- one point light: distances, facing, GGX degenerate half vector, the miss, the selection draw with one light
    L1 = [light()]
    lp = np.array(L1[0]["posW"], F)
    z = np.zeros(n, np.int64)
    parts = {"ordinary_point": (_around(rng, L1, z, n), z)}
    # distance^2 on either side of 1e-5 (offsets along one axis: d2 = x * x exactly), and exactly 0
    x = np.sqrt(np.float64(F(1e-5))) * (1.0 + rng.uniform(-3e-7, 3e-7, n))
    x[::8] = 0.0
    axis = cyc(3)
    off = np.zeros((n, 3), F)
    off[np.arange(n), axis] = (x * np.where(cyc(2) == 0, 1, -1)).astype(F)
    s = _surface_at(rng, (lp + off).astype(F), -off)
    parts["dist2_threshold"] = (s, z)
    # distance^2 overflows: 1e20 away (the case one_point_tiny has the one that underflows)
    far = _around(rng, L1, z, n, 1e20, 1e20)
    parts["dist2_overflow"] = (far, z)
    # N.L == 0: N in the plane perpendicular to the offset, exactly: offset along z, N = (c, s, 0)
    a = rng.uniform(0, 2 * np.pi, n)
    off = np.zeros((n, 3), F)
    off[:, 2] = -rng.uniform(0.5, 2.0, n).astype(F)
    s = _surface_at(rng, (lp + off).astype(F))
    s[:, 4:7] = np.stack([np.cos(a), np.sin(a), np.zeros(n)], axis=1).astype(F)
    parts["nl_zero"] = (s, z)
    s = _around(rng, L1, z, n)
    s[:, 4:7] = -s[:, 4:7]
    parts["back_facing"] = (s, z)
    # GGX with V == -L: V is the negated fp32 direction to the light as getLightData forms it
    s = _around(rng, L1, z, n)
    s[:, 8:11] = np.negative(normalize3(normalize3((lp[None] - s[:, 0:3]).astype(F))))
    parts["v_is_minus_l"] = (s, z)
    s = _around(rng, L1, z, n)
    s.view(np.int32)[:, 23] = -1
    s[::2, 0:3] = np.nan
    parts["miss"] = (s, z)
    c = _case("one_point", L1, parts, rng, ill=("dist2_threshold", "dist2_overflow", "nl_zero"))
    # the selection draw with one light: r * 1 is r; draws of 0 and of 1 - 2^-24
    m = c.of("ordinary_point")
    low = np.where(np.arange(int(m.sum())) % 2 == 0, 0, TOP24).astype(np.uint64)
    c.seeds[m] = seeds_with_draw(rng, low, 1)
    cases.append(c)

    # -- a tiny distance: the light sits 1e-30 from the points, so (lightPos - posW)^2 underflows to 0
    Lt = [light(pos=(0.0, 0.0, 0.0))]
    off = unit(rng, n) * F(1e-30)
    cases.append(_case("one_point_tiny", Lt, {"dist2_underflow": (_surface_at(rng, off.astype(F), -off), z)}, rng, ill=()))

    # -- the cone's edge: three spot lights that differ in cosOpeningAngle only: the fp32 cosTheta of every record of the
    # family is that of one fixed offset direction, and cosOpeningAngle is that value, one step above and one step below
    th0 = 0.4
    o = np.array([np.sin(th0), 0.0, -np.cos(th0)], F)
    cos_t = float(normalize3(np.negative(o)[None])[0, 2])  # cosTheta = -dot(lsL, (0, 0, -1)) = lsL.z, lsL = normalize(-o * t)
    spots = [light(opening=th0, cos_opening=cc, penumbra=0.0) for cc in (cos_t, float(step(F(cos_t), 1)), float(step(F(cos_t), -1)))]
    w3 = cyc(3).astype(np.int64)
    t = rng.uniform(0.5, 3.0, 8 * n).astype(F)
    pos = (np.array(spots[0]["posW"], F)[None] + o[None] * t[:, None]).astype(F)
    # (the sum rounds, so the direction the kernel sees is re-derived and only rows that kept the bits stay in the family)
    lsl = normalize3((np.array(spots[0]["posW"], F)[None] - pos).astype(F))
    keep = np.nonzero(lsl[:, 2] == F(cos_t))[0][:n]
    s = _surface_at(rng, pos[keep], -np.tile(o[None], (len(keep), 1)))
    parts = {"cone_edge": (s, cyc(3, len(keep)).astype(np.int64)), "cone_inside_outside": (_in_cone(rng, spots, w3, n, 0.8), w3)}
    cases.append(_case("cone_edge", spots, parts, rng, ill=("cone_edge",)))

    # -- penumbra: 0, 1e-30, equal to openingAngle and larger than it
    pen = [light(opening=0.6, penumbra=p) for p in (0.0, 1e-30, 0.6, 0.9)]
    w4 = cyc(4).astype(np.int64)
    cases.append(_case("penumbra", pen, {"penumbra": (_in_cone(rng, pen, w4, n, 0.9), w4)}, rng, ill=()))

    # -- openingAngle 0 and pi, a spot light with a zero-length dirW and one with a non-unit dirW
    odd = [light(opening=0.0), light(opening=np.pi), light(opening=0.6, direction=(0, 0, 0), penumbra=0.2),
           light(opening=0.6, direction=(0, 0, -3.0), penumbra=0.2)]
    s = _in_cone(rng, odd, w4, n, 0.9)
    on_axis = (w4 == 0) & (np.arange(n) % 8 < 4)  # openingAngle 0: only the axis itself is inside
    s[on_axis, 0:2] = np.array(odd[0]["posW"], F)[None, 0:2]
    cases.append(_case("opening_and_dir", odd, {"opening_and_dir": (s, w4)}, rng, ill=("opening_and_dir",)))

    # -- directional lights: unit, zero-length and non-unit dirW
    dirs = [light(LIGHT_DIRECTIONAL, direction=(0.0, -0.6, -0.8)), light(LIGHT_DIRECTIONAL, direction=(0, 0, 0)),
            light(LIGHT_DIRECTIONAL, direction=(0.0, -1.8, -2.4))]
    pos = rng.uniform(-2, 2, (n, 3)).astype(F)
    pos[::16] = np.array(dirs[0]["posW"], F)  # the point at the light's posW: the distance of lsPos is 0
    s = _surface_at(rng, pos, np.tile(np.array([[0.0, 0.6, 0.8]], F), (n, 1)))
    cases.append(_case("directional", dirs, {"directional": (s, w3)}, rng, ill=()))

    # -- intensities 0, negative, 1e30 and inf
    ints = [light(intensity=i) for i in ((0, 0, 0), (-1.0, -2.0, 0.5), (1e30, 1e30, 1e30), (np.inf, 1.0, np.inf))]
    cases.append(_case("intensity", ints, {"intensity": (_around(rng, ints, w4, n), w4)}, rng, ill=()))

    # -- the selection draw: r * lightsCount exactly integral, one step to either side, and the last light
    for count in (3, 4):
        ls = [light(pos=(0.25 + 0.5 * k, 0.5, 2.0), intensity=(1.0 + k, 2.0, 3.0)) for k in range(count)]
        low = []
        for k in range(count + 1):
            c0 = int(round(k * 2 ** 24 / count))
            low += [c0 - 1, c0, c0 + 1]
        low = np.array([v for v in low if 0 <= v <= TOP24] + [TOP24, 0], np.uint64)
        low = low[np.arange(n) % len(low)]
        sd = seeds_with_draw(rng, low, 1)
        _, r = lcg(sd)
        which = np.minimum((r * F(count)).astype(np.int64), count - 1)
        c = _case(f"selection_{count}", ls, {"selection": (_around(rng, ls, which, n), which)}, rng, ill=("selection",))
        order = np.argsort(np.argsort(c.which, kind="stable"), kind="stable")  # (the interleave permuted the rows: match seeds to `which`)
        by_which = np.argsort(which, kind="stable")
        c.seeds = np.ascontiguousarray(sd[by_which][order], np.uint32)
        _, r = lcg(c.seeds)
        assert np.array_equal(np.minimum((r * F(count)).astype(np.int64), count - 1), c.which)
        cases.append(c)
    return cases


# ---- connection records: vertex pairs ---------------------------------------------------------------------------------
class VertexRecords(Batch):
    def __init__(self, d, family, names):
        super().__init__(family, names)
        self.eye, self.light = np.ascontiguousarray(d["eye"], F), np.ascontiguousarray(d["light"], F)
        self.eye_prev, self.light_prev = np.ascontiguousarray(d["eye_prev"], F), np.ascontiguousarray(d["light_prev"], F)
        self.eye_spec, self.light_spec = np.ascontiguousarray(d["eye_spec"], np.uint8), np.ascontiguousarray(d["light_spec"], np.uint8)
        self.n = len(self.eye)


def _pair(rng, n, gap=None):
    """ordinary pairs: two surfaces facing each other, a predecessor on each one's own side"""
    pe = rng.uniform(-1, 1, (n, 3)).astype(F)
    sep = unit(rng, n) * (rng.uniform(0.3, 2.0, (n, 1)).astype(F) if gap is None else gap)
    pl = (pe + sep).astype(F)
    eye, lig = _surface_at(rng, pe, pl - pe), _surface_at(rng, pl, pe - pl)
    eprev = (pe + eye[:, 8:11] * rng.uniform(0.5, 2.0, (n, 1)).astype(F)).astype(F)
    lprev = (pl + lig[:, 8:11] * rng.uniform(0.5, 2.0, (n, 1)).astype(F)).astype(F)
    z = np.zeros((n, 1), F)
    return dict(eye=eye, light=lig, eye_prev=np.concatenate([eprev, z], axis=1), light_prev=np.concatenate([lprev, z], axis=1),
                eye_spec=rng.integers(0, 2, n).astype(np.uint8), light_spec=rng.integers(0, 2, n).astype(np.uint8))


def vertex_families(seed=1, n=FAMILY_N):
    rng = np.random.default_rng(seed + 3000)
    fam = {}

    def new(name, gap=None):
        fam[name] = _pair(rng, n, gap)
        return fam[name]

    new("ordinary")
    d = new("coincident")
    d["light"][:, 0:3] = d["eye"][:, 0:3]
    d = new("one_step_apart")
    d["light"][:, 0:3] = d["eye"][:, 0:3]
    ax = np.arange(n) % 3
    d["light"][np.arange(n), ax] = np.nextafter(d["eye"][np.arange(n), ax], F(np.inf))
    # 1e-20 apart (around the origin, where fp32 resolves it): invLengthAB^2 overflows
    d = new("apart_1e-20")
    d["eye"][:, 0:3] = 0.0
    d["light"][:, 0:3] = normalize3((d["light"][:, 0:3] - d["eye"][:, 0:3]).astype(F)) * F(1e-20)
    new("apart_1e15", gap=F(1e15))
    new("apart_1e20", gap=F(1e20))  # length^2 overflows: invLengthAB is 0
    # both cosines 0: each normal exactly perpendicular to the (axis-aligned) connection
    d = new("tangent_planes")
    k = np.arange(n)
    d["light"][:, 0:3] = d["eye"][:, 0:3]
    d["light"][k, ax] = d["eye"][k, ax] + rng.uniform(0.5, 2.0, n).astype(F)
    for side in ("eye", "light"):
        d[side][k, 4 + ax] = 0.0
    # connectDir == +-woL: the light vertex's predecessor lies on the connection line, on the eye's side or beyond
    d = new("connectdir_is_wol")
    # The light vertex sits at the origin, so that eye - light, prev - light and their negations are exact and the
    # outgoing direction equals +-connectDir bit for bit, from V and from the predecessor alike.  Rows by k % 4:
    #   0  woL = +connectDir (predecessor = the eye vertex): H = connectDir, L.H = 1
    #   1  woL = -connectDir, N towards the eye: the cosine test cuts fsL to 0
    #   2  woL = -connectDir, N away from the eye, specular lobe: H = normalize(0), fsL is NaN
    #   3  as 2 with the diffuse lobe: fsL = dif / pi
    sep = (d["eye"][:, 0:3] - d["light"][:, 0:3]).astype(F)
    d["light"][:, 0:3] = 0.0
    d["eye"][:, 0:3] = sep
    sgn = np.where(k % 4 == 0, 1, -1).astype(F)[:, None]
    d["light_prev"][:, 0:3] = sgn * sep
    d["light"][:, 8:11] = sgn * normalize3(sep)
    away = k % 4 >= 2
    d["light"][away, 4:7] = -d["light"][away, 4:7]
    d["light_spec"][k % 4 == 2] = 1
    d["light_spec"][k % 4 == 3] = 0
    d["eye_prev"][:, 0:3] = (sep + d["eye"][:, 8:11]).astype(F)
    d = new("prev_is_vertex")
    d["eye_prev"][::2, 0:3] = d["eye"][::2, 0:3]
    d["light_prev"][1::2, 0:3] = d["light"][1::2, 0:3]
    d = new("black")
    d["eye"][::2, 12:15] = d["eye"][::2, 16:19] = 0.0
    d["light"][1::2, 12:15] = d["light"][1::2, 16:19] = 0.0
    d = new("fsl_zero")  # the light vertex faces away from its predecessor: evalBRDF's cosine test gives fsL = 0
    d["light"][:, 8:11] = -d["light"][:, 4:7]
    d["light_prev"][:, 0:3] = (d["light"][:, 0:3] - d["light"][:, 4:7]).astype(F)
    d = new("fse_zero")
    d["eye"][:, 8:11] = -d["eye"][:, 4:7]
    d["eye_prev"][:, 0:3] = (d["eye"][:, 0:3] - d["eye"][:, 4:7]).astype(F)
    d = new("spec_flags")
    d["eye_spec"][:] = (k % 4) // 2
    d["light_spec"][:] = k % 2
    d = new("miss")
    d["eye"].view(np.int32)[::2, 23] = -1
    d["light"].view(np.int32)[1::3, 23] = -1
    d["eye"][::4, 4:7] = np.nan
    return fam


VERTEX_ILL = ("coincident", "one_step_apart", "apart_1e-20", "apart_1e20", "tangent_planes", "connectdir_is_wol", "prev_is_vertex",
              "fsl_zero", "fse_zero")


def vertex_records(name, seed=1):
    d = vertex_families(seed)[name]
    return VertexRecords(d, np.zeros(len(d["eye"]), np.int32), [name])


def vertex_mixed(seed=1):
    fam = vertex_families(seed)
    rng = np.random.default_rng(seed + 3500)
    fam["random"] = _pair(rng, sum(len(v["eye"]) for v in fam.values()))
    d, label, names = _interleave(fam, rng)
    return VertexRecords(d, label, names)


# ---- connection records: light vertices against a camera ---------------------------------------------------------------
FRAMES = ((17, 9, (0.0, 0.0)), (16, 8, (0.0, 0.0)), (17, 9, (0.375, -0.25)), (16, 8, (-0.4375, 0.3125)))  # W, H, pixel jitter


def origin_camera(abi):
    """A camera at the origin (where fp32 resolves positions far finer than a pixel coordinate's last bit) with the Cornell
    camera's axes and field of view: an axis-aligned cameraW lets a depth of 1e-40 arrive as a subnormal d3"""
    c, sn = 1.0, 0.0
    cam = abi.Camera()
    for k, v in enumerate((0.0, 0.0, 0.0)):
        cam.posW[k] = v
    for k, v in enumerate((-0.675 * c, 0.0, -0.675 * sn)):
        cam.cameraU[k] = v
    for k, v in enumerate((0.0, 0.357, 0.0)):
        cam.cameraV[k] = v
    for k, v in enumerate((-sn, 0.0, c)):
        cam.cameraW[k] = v
    return cam


def camera_of(cam):
    """(pos, U, V, W) fp32 arrays of a bdpt_camera"""
    return tuple(np.array(getattr(cam, k)[:], F) for k in ("posW", "cameraU", "cameraV", "cameraW"))


def splat_target32(cam, pos, W, H, jit):
    """splatTarget (device_connect.hpp) in fp32 numpy: (facing, px * W - jx, py * H - jy, fx, fy, inside, d3)"""
    cpos, U, V, Wc = cam
    one = lambda v: np.broadcast_to(v[None], pos.shape)  # noqa: E731
    with np.errstate(all="ignore"):
        d = normalize3((cpos[None] - pos).astype(F))
        cn = normalize3(Wc[None])[0]
        facing = dot3(one(cn), d) < 0
        d1 = dot3(d, one(U)) / dot3(U, U)
        d2 = dot3(d, one(V)) / dot3(V, V)
        d3 = dot3(d, one(Wc)) / dot3(Wc, Wc)
        px, py = (d1 / d3) * F(0.5) + F(0.5), (-d2 / d3) * F(0.5) + F(0.5)
        gx, gy = px * F(W) - F(jit[0]), py * F(H) - F(jit[1])
        fx, fy = np.rint(gx), np.rint(gy)
        inside = facing & (fx >= 0) & (fx < W) & (fy >= 0) & (fy < H)
    return facing, gx, gy, fx, fy, inside, d3


def _camera_points(cam, sx, sy, depth):
    """points in front of the camera at screen coordinates (sx, sy) in [-1, 1]^2 (x right, y up) and the given depth
    along cameraW (float64; the caller rounds)"""
    cpos, U, V, Wc = (a.astype(np.float64) for a in cam)
    return cpos[None] + depth[:, None] * (Wc[None] + sx[:, None] * U[None] + sy[:, None] * V[None])


def _solve_gx(cam, W, H, jit, want, sy, depth, axis=0):
    """screen coordinates (along `axis`; the other one fixed at sy) whose fp32 px * W - jx (py * H - jy) is as close to
    `want` as a bisection over the coordinate gets: many land on it exactly"""
    size = (W, H)[axis]
    lo, hi = np.full(len(want), -1.5), np.full(len(want), 1.5)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        s = (mid, sy) if axis == 0 else (sy, mid)
        g = splat_target32(cam, _camera_points(cam, s[0], s[1], depth).astype(F), W, H, jit)[1 + axis]
        below = g < want if axis == 0 else g > want  # (py falls as the point rises)
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    return 0.5 * (lo + hi), size


def _snap(cam, W, H, jit, pos, want, axis):
    """fp32 positions nudged by up to 24 steps in one coordinate so that px * W - jx (py * H - jy) equals `want` bit for
    bit wherever some nudge does that (the bisection alone ends a rounding or two away)"""
    pos = np.ascontiguousarray(pos, F)
    out, done = pos.copy(), splat_target32(cam, pos, W, H, jit)[1 + axis] == want
    for comp in range(3):
        for k in range(-24, 25):
            cand = pos.copy()
            cand[:, comp] = step(pos[:, comp], k)
            hit = (splat_target32(cam, cand, W, H, jit)[1 + axis] == want) & ~done
            out[hit], done = cand[hit], done | hit
    return out


class CameraRecords(Batch):
    def __init__(self, d, family, names, W, H, jit):
        super().__init__(family, names)
        self.light, self.light_spec = np.ascontiguousarray(d["light"], F), np.ascontiguousarray(d["light_spec"], np.uint8)
        self.n, self.W, self.H, self.jit = len(self.light), W, H, jit


def camera_families(cam, W, H, jit, seed=1, n=FAMILY_N):
    """cam: (pos, U, V, W) of camera_of.  Light vertices whose splat target sits on the frame's edges, on rintf ties, ..."""
    rng = np.random.default_rng(seed + 4000 + W)
    fam = {}
    cpos, U, V, Wc = cam
    ext = float(np.linalg.norm(Wc))

    def put(name, pos):
        pos = np.ascontiguousarray(pos, F)
        with np.errstate(all="ignore"):
            s = _surface_at(rng, pos, np.nan_to_num((cpos[None] - pos).astype(F)))
        fam[name] = dict(light=s, light_spec=rng.integers(0, 2, len(pos)).astype(np.uint8))
        return fam[name]

    depth = rng.uniform(0.5, 3.0, n)
    put("ordinary", _camera_points(cam, rng.uniform(-1.2, 1.2, n), rng.uniform(-1.2, 1.2, n), depth))
    # the frame's edges and corners: px * W - jx at -0.5, W - 0.5 (the rintf boundaries of the first and last column),
    # py likewise, each approached by bisection, so that rows fall on both sides and on the boundary
    k = np.arange(n)
    wx = np.array([-0.5, W - 0.5, 0.0, W - 1.0, float(W)], F)[k % 5]
    wy = np.array([-0.5, H - 0.5, 0.0, H - 1.0, float(H)], F)[(k // 5) % 5]
    sy0 = rng.uniform(-0.9, 0.9, n)
    off = np.where(k % 4 == 1, 3e-7, np.where(k % 4 == 3, -3e-7, 0.0))  # (the bisection ends on one side: the other side too)
    sx, _ = _solve_gx(cam, W, H, jit, wx, sy0, depth, 0)
    sx = sx + off
    half = k % 2 == 0  # every other row is left where the bisection ended: a rounding or two off the boundary, either side
    snap = lambda pos, want, axis: np.where(half[:, None], _snap(cam, W, H, jit, pos, want, axis), pos.astype(F))  # noqa: E731
    put("edge_x", snap(_camera_points(cam, sx, sy0, depth), wx, 0))
    sy, _ = _solve_gx(cam, W, H, jit, wy, sy0, depth, 1)
    sy = sy + off
    put("edge_y", snap(_camera_points(cam, sy0, sy, depth), wy, 1))
    sxc, _ = _solve_gx(cam, W, H, jit, wx, sy, depth, 0)
    sxc = sxc + off
    put("corner", snap(_camera_points(cam, sxc, sy, depth), wx, 0))
    # rintf ties: px * W - jx = k + 0.5 for even and odd k
    tx = (rng.integers(0, W - 1, n) + 0.5).astype(F)
    sx, _ = _solve_gx(cam, W, H, jit, tx, sy0, depth, 0)
    put("tie_x", snap(_camera_points(cam, sx, sy0, depth), tx, 0))
    ty = (rng.integers(0, H - 1, n) + 0.5).astype(F)
    sy, _ = _solve_gx(cam, W, H, jit, ty, sy0, depth, 1)
    put("tie_y", snap(_camera_points(cam, sy0, sy, depth), ty, 1))
    # in the camera plane (dot(cameraN, dir) == 0 or a rounding away from it: d3 is 0 or tiny, nx = +-inf or NaN), behind
    # the camera, at the camera, 1e20 away
    su, sv = rng.uniform(-2, 2, n), rng.uniform(-2, 2, n)
    tiny = np.array([0.0, 1e-40, 1e-30, -1e-40, 1e-20], np.float64)[k % 5]  # depth: d3 is 0, subnormal, tiny, or behind
    put("camera_plane", cpos[None].astype(np.float64) + su[:, None] * U[None] + sv[:, None] * V[None] + tiny[:, None] * Wc[None])
    put("behind", _camera_points(cam, rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), -depth))
    d = put("at_camera", np.tile(cpos[None], (n, 1)))
    d["light"][1::2, 0:3] = np.nextafter(d["light"][1::2, 0:3], F(np.inf))
    put("far_1e20", _camera_points(cam, rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), np.full(n, 1e20 / ext)))
    # GGX with V == -dirToCamera (the fp32 direction the kernel forms) and the specular lobe: H = normalize(0)
    d = put("v_is_minus_dir", _camera_points(cam, rng.uniform(-0.9, 0.9, n), rng.uniform(-0.9, 0.9, n), depth))
    d["light"][:, 8:11] = np.negative(normalize3((cpos[None] - d["light"][:, 0:3]).astype(F)))
    d["light_spec"][:] = 1
    d = put("miss", _camera_points(cam, rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), depth))
    d["light"].view(np.int32)[:, 23] = -1
    d["light"][::2, 0:3] = np.nan
    return fam


CAMERA_ILL = ("edge_x", "edge_y", "corner", "tie_x", "tie_y", "camera_plane", "at_camera", "far_1e20", "v_is_minus_dir")


def camera_mixed(cam, W, H, jit, seed=1):
    fam = camera_families(cam, W, H, jit, seed)
    rng = np.random.default_rng(seed + 4500)
    m = sum(len(v["light"]) for v in fam.values())
    pos = _camera_points(cam, rng.uniform(-1.2, 1.2, m), rng.uniform(-1.2, 1.2, m), rng.uniform(0.5, 3.0, m)).astype(F)
    fam["random"] = dict(light=_surface_at(rng, pos, (cam[0][None] - pos).astype(F)), light_spec=rng.integers(0, 2, m).astype(np.uint8))
    d, label, names = _interleave(fam, rng)
    return CameraRecords(d, label, names, W, H, jit)


# ---- the two-triangle scene of the light tests ---------------------------------------------------------------------------
def two_triangle_scene(abi, num_lights):
    """One opaque unit quad in z = 0 and num_lights point lights (placeholders: the tests set their own with
    bdpt_set_lights, which keeps the count).  -> (desc, the arrays it points into)"""
    pos = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], F)
    nrm = np.tile(np.array([[0, 0, 1]], F), (4, 1))
    uv = np.ascontiguousarray(pos.copy())
    idx = np.array([0, 1, 2, 0, 2, 3], np.uint32)
    tri_mat = np.zeros(2, np.uint32)
    mats = (abi.Material * 1)()
    for k in range(4):
        mats[0].baseColor[k] = 1.0
    mats[0].alphaThreshold = 0.5
    mats[0].IoR = 1.5
    mats[0].flags = (1 << 3) | (1 << 6) | (1 << 19)  # the opaque material of edge_rays.grid_desc
    mats[0].texBaseColor = mats[0].texSpecular = mats[0].texEmissive = mats[0].texNormal = -1
    lights = make_lights(abi, [light(pos=(0.5, 0.5, 1.0 + k)) for k in range(num_lights)])
    d = abi.SceneDesc()
    d.numVertices, d.numTriangles, d.numMaterials, d.numTextures, d.numLights = 4, 2, 1, 0, num_lights
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    d.positions, d.normals, d.texcoords = fp(pos), fp(nrm), fp(uv)
    d.indices = idx.ctypes.data_as(C.POINTER(C.c_uint32))
    d.triMaterial = tri_mat.ctypes.data_as(C.POINTER(C.c_uint32))
    d.materials, d.lights = mats, lights
    return d, [pos, nrm, uv, idx, tri_mat, mats, lights]
