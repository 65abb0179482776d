"""Scenes and oracle calls shared by the area-light tests (BDPT_PARAM_AREA_LIGHTS; contract: include/bdpt.h "Area lights").

AreaScene is the Cornell box with emitters; emitter_soup builds tables of any size; the oracle_area_* functions call the
area-light entry points of oracle/liboracle.so."""
import ctypes as C
import math

import numpy as np

from area_light_numpy import AreaTable

AREA = 4096
NO_NEE, NO_SPLAT, NO_CONNECT, MIS_POWER, ENV_ON_MISS, EMISSIVE_HITS = 4, 8, 16, 64, 1024, 2048
DEFER_RESOLVE, DEFER_TAIL = 2, 256


def _flags(dif, spec, emis, alpha=0):
    return (dif << 3) | (spec << 6) | (emis << 9) | (alpha << 17)


def _arr(ptr, n, dtype):
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype).copy()


def bits(t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _quad(x, y, z, up=False):
    """(4 corners, 2 triangles) of an axis-aligned quad at height y; the winding gives n_g = -y, or +y with up"""
    (x0, x1), (z0, z1) = x, z
    q = np.array([[x0, y, z0], [x1, y, z0], [x1, y, z1], [x0, y, z1]], np.float32)
    tris = np.array([[0, 2, 1], [0, 3, 2]] if up else [[0, 1, 2], [0, 2, 3]], np.uint32)
    return q, tris


def copy_desc(pkg, desc):
    """Copies of a scene description's arrays: dict of P, N, T (zeros without texcoords), B (None without bitangents),
    I (n x 3), M, mats (a list of bdpt_material), textures ((H x W x 4 uint8, srgb) pairs), lights (a list)"""
    a, d = pkg.abi, desc
    nv, nt = int(d.numVertices), int(d.numTriangles)
    v3 = lambda ptr: _arr(ptr, nv * 3, np.float32).reshape(-1, 3)
    mats = [a.Material() for _ in range(int(d.numMaterials))]
    for i, m in enumerate(mats):
        C.memmove(C.byref(m), C.byref(d.materials[i]), C.sizeof(a.Material))
    lights = [a.Light() for _ in range(int(d.numLights))]
    for i, l in enumerate(lights):
        C.memmove(C.byref(l), C.byref(d.lights[i]), C.sizeof(a.Light))
    textures = [(np.ctypeslib.as_array(d.textures[k].rgba8, shape=(d.textures[k].height, d.textures[k].width, 4)).copy(),
                 bool(d.textures[k].srgb)) for k in range(int(d.numTextures))]
    return dict(P=v3(d.positions), N=v3(d.normals), T=v3(d.texcoords) if d.texcoords else np.zeros((nv, 3), np.float32),
                B=v3(d.bitangents) if d.bitangents else None, I=_arr(d.indices, nt * 3, np.uint32).reshape(-1, 3),
                M=_arr(d.triMaterial, nt, np.uint32), mats=mats, textures=textures, lights=lights)


class DescArrays:
    """A bdpt_scene_desc over numpy arrays and ctypes tables it keeps alive."""

    def __init__(self, a, P, N, T, I, M, mats, textures, lights, B=None):
        self.P, self.N, self.T, self.I, self.M = (np.ascontiguousarray(x) for x in (P, N, T, I, M))
        self.B = None if B is None else np.ascontiguousarray(B, np.float32)
        self.textures = list(textures)
        self.mats = (a.Material * len(mats))(*mats)
        self._tex_c = (a.Texture * max(len(self.textures), 1))()
        for k, (t, srgb) in enumerate(self.textures):
            self._tex_c[k].rgba8 = t.ctypes.data_as(C.POINTER(C.c_uint8))
            self._tex_c[k].width, self._tex_c[k].height, self._tex_c[k].srgb = t.shape[1], t.shape[0], int(srgb)
        self.lights = (a.Light * len(lights))(*lights)
        self.desc = a.SceneDesc()
        dd = self.desc
        dd.numVertices, dd.numTriangles, dd.numMaterials = self.P.shape[0], self.I.shape[0], len(mats)
        dd.numTextures, dd.numLights = len(self.textures), len(lights)
        f = C.POINTER(C.c_float)
        dd.positions, dd.normals, dd.texcoords = (x.ctypes.data_as(f) for x in (self.P, self.N, self.T))
        dd.bitangents = None if self.B is None else self.B.ctypes.data_as(f)
        dd.indices = self.I.ctypes.data_as(C.POINTER(C.c_uint32))
        dd.triMaterial = self.M.ctypes.data_as(C.POINTER(C.c_uint32))
        dd.materials = C.cast(self.mats, C.POINTER(a.Material))
        dd.textures = C.cast(self._tex_c, C.POINTER(a.Texture)) if self.textures else None
        dd.lights = C.cast(self.lights, C.POINTER(a.Light))

    def table(self, dropped=()):
        return AreaTable(self.P, self.I, self.M, list(self.mats), self.textures, self.T, dropped=dropped)


def _light(a, typ, pos, direction, intensity, opening=math.pi, penumbra=0.0):
    l = a.Light()
    l.type = typ
    n = math.sqrt(sum(x * x for x in direction))
    for k in range(3):
        l.posW[k], l.dirW[k], l.intensity[k] = pos[k], direction[k] / n, intensity[k]
    l.openingAngle, l.cosOpeningAngle, l.penumbraAngle = opening, math.cos(opening), penumbra
    return l


class AreaScene(DescArrays):
    """The Cornell box (camera: the base scene's) with its emissive ceiling patch and
      extra=True:        a floating textured emitter and a floating alpha-masked emitter (checker of alpha 255 / 0);
      const_extra=True:  two more constant emitters of other luminances, the second facing up (the floor sees its back);
      transparent=True:  a fully transparent alpha-masked emissive quad, which the device build drops (self.dropped);
      point_light=True:  the box's point light as it is (else its intensity is 0: every point-light term is +0);
      relit=True:        a spot light with a penumbra, a second point light and a directional light inside the box."""

    def __init__(self, pkg, base, positions=None, patch_emission=None, extra=True, const_extra=False, transparent=False,
                 point_light=False, relit=False):
        a = pkg.abi
        c = copy_desc(pkg, base.desc)
        P, N, T, I, M, mats = c["P"], c["N"], c["T"], c["I"], c["M"], c["mats"]
        if patch_emission is not None:
            for k in range(3):
                mats[3].emissive[k] = patch_emission[k]

        def new_mat(flags, emissive=(0.0, 0.0, 0.0)):
            m = a.Material()
            m.baseColor[:] = (0.6, 0.6, 0.6, 1.0)
            m.specular[:] = (0.0, 1.0, 0.0, 0.0)  # roughness 1, metallic 0
            m.alphaThreshold, m.IoR = 0.5, 1.5
            m.texBaseColor = m.texSpecular = m.texEmissive = m.texNormal = -1
            m.flags = flags
            m.emissive[:] = emissive
            mats.append(m)
            return len(mats) - 1

        textures = []
        quads = []  # (x range, z range, y, material, facing up)
        if extra:
            # textured emitter: a constant sRGB texel; alpha-masked emitter: alpha 255 / 0 in a 2x2 checker of 2x2 blocks
            tex_e = np.zeros((4, 4, 4), np.uint8)
            tex_e[...] = (200, 150, 100, 255)
            tex_a = np.full((4, 4, 4), 128, np.uint8)
            yy, xx = np.mgrid[0:4, 0:4]
            tex_a[..., 3] = np.where(((yy // 2) + (xx // 2)) % 2 == 0, 255, 0)
            textures += [(tex_e, True), (tex_a, False)]
            m_tex = new_mat(_flags(1, 1, 2))
            mats[m_tex].texEmissive = 0
            m_alpha = new_mat(_flags(2, 1, 1, alpha=1), (2.0, 1.5, 1.0))
            mats[m_alpha].texBaseColor = 1
            quads += [((80, 200), (150, 300), 420.0, m_tex, False), ((330, 480), (300, 450), 350.0, m_alpha, False)]
        if const_extra:
            quads += [((60, 160), (360, 480), 400.0, new_mat(_flags(1, 1, 1), (3.0, 2.0, 1.0)), False),
                      ((380, 500), (90, 200), 250.0, new_mat(_flags(1, 1, 1), (0.5, 1.0, 2.0)), True)]
        self.dropped = []
        m_t = None
        if transparent:
            tex_t = np.full((2, 2, 4), 160, np.uint8)
            tex_t[..., 3] = 0
            textures.append((tex_t, False))
            m_t = new_mat(_flags(2, 1, 1, alpha=1), (4.0, 4.0, 4.0))
            mats[m_t].texBaseColor = len(textures) - 1
            quads.append(((200, 320), (180, 300), 300.0, m_t, False))
        for (x0, x1), (z0, z1), y, mid, up in quads:
            q, tris = _quad((x0, x1), y, (z0, z1), up)
            if mid == m_t:
                self.dropped += [I.shape[0], I.shape[0] + 1]
            base_v = P.shape[0]
            P = np.concatenate([P, q])
            N = np.concatenate([N, np.tile([[0, 1 if up else -1, 0]], (4, 1)).astype(np.float32)])
            T = np.concatenate([T, np.array([[0, 0, 0], [1.25, 0, 0], [1.25, 1.25, 0], [0, 1.25, 0]], np.float32)])
            I = np.concatenate([I, tris + base_v])
            M = np.concatenate([M, np.array([mid, mid], np.uint32)])
        # the ceiling patch 10 units lower than the box's 0.1 below the ceiling: the ceiling next to it then sees its top side
        # from no closer than that, which keeps NEE's 1 / d^2 tail (and so the sample variances the block test relies on) bounded
        P[np.unique(I[M == 3])] -= np.array([0.0, 10.0, 0.0], np.float32)
        if positions is not None:
            P[: positions.shape[0]] = positions
        light = c["lights"][0]
        I0 = [float(light.intensity[k]) for k in range(3)]
        if not point_light:
            light.intensity[0] = light.intensity[1] = light.intensity[2] = 0.0
        lights = [light]
        if relit:
            s = max(I0) if max(I0) > 0 else 1.0
            lights += [_light(a, a.LIGHT_POINT, (278.0, 520.0, 260.0), (0.1, -1.0, 0.15), (0.9 * s, 0.8 * s, 0.6 * s),
                              opening=0.6, penumbra=0.2),
                       _light(a, a.LIGHT_POINT, (120.0, 150.0, 420.0), (0.0, -1.0, 0.0), (0.3 * s, 0.35 * s, 0.5 * s)),
                       _light(a, a.LIGHT_DIRECTIONAL, (300.0, 400.0, 300.0), (0.3, -1.0, 0.25), (0.5, 0.45, 0.4))]
        super().__init__(a, P, N, T, I, M, mats, textures, lights)
        self.base = base

    def camera(self, aspect):
        return self.base.camera(aspect)


def emitter_soup(pkg, n_emitters, seed=0, tail_zero=8, with_point_light=True):
    """About n_emitters emitters among as many other triangles, for tables of any size: random small triangles in a
    100-unit box, in groups that mix constant emitters of two luminances, a textured emitter (a 5x3 texture, UVs that
    wrap), non-emitters and zero-luminance emitter materials, so that waves of 64 straddle the compaction.  Every 97th
    emitter has zero area, and the last `tail_zero` emitters (a run at the end of the table) have zero area too."""
    a = pkg.abi
    rng = np.random.default_rng(seed)
    tex = rng.integers(0, 256, (3, 5, 4), dtype=np.uint8)
    tex[..., 3] = 255

    def mat(emis_type, emissive=(0.0, 0.0, 0.0), tex_emissive=-1):
        m = a.Material()
        m.baseColor[:] = (0.5, 0.5, 0.5, 1.0)
        m.specular[:] = (0.0, 0.5, 0.0, 0.0)
        m.alphaThreshold, m.IoR = 0.5, 1.5
        m.texBaseColor = m.texSpecular = m.texNormal = -1
        m.texEmissive = tex_emissive
        m.flags = _flags(1, 1, emis_type)
        m.emissive[:] = emissive
        return m

    mats = [mat(1, (1.0, 0.8, 0.6)), mat(1, (5.0, 5.0, 5.0)), mat(2, tex_emissive=0), mat(1), mat(0, (3.0, 3.0, 3.0))]
    emitter_mats = (0, 1, 2)
    kinds = []
    made = 0
    while made < n_emitters:
        r = rng.random()
        if r < 0.45:
            kinds.append(int(rng.choice(emitter_mats)))
            made += 1
        else:
            kinds.append(int(rng.choice((3, 4))))  # zero-luminance constant emission, or no emissive channel
        if rng.random() < 0.01:  # now and then a whole run of non-emitters: a wave without any emitter
            kinds += [3] * int(rng.integers(60, 200))
    nt = len(kinds)
    # corners c + (u sx, 0, 0), c + (0, v sy, 0), c + (0, 0, w sz): the cross product has no cancelling terms, so the fp32
    # area is within a few ulp of the exact one
    c = rng.uniform(0.0, 100.0, (nt, 1, 3))
    P = np.repeat(c, 3, axis=1)
    P[:, [0, 1, 2], [0, 1, 2]] += rng.uniform(0.3, 1.2, (nt, 3)) * rng.choice((-1.0, 1.0), (nt, 3))
    P = P.astype(np.float32)
    em = [t for t, k in enumerate(kinds) if k in emitter_mats]
    flat = em[96::97] + em[len(em) - tail_zero:]
    for t in flat:
        P[t, 2] = P[t, t % 2]  # a repeated corner: zero area, exactly
    P = P.reshape(-1, 3)
    Nn = np.tile(np.array([[0.0, 1.0, 0.0]], np.float32), (P.shape[0], 1))
    T = np.zeros((P.shape[0], 3), np.float32)
    T[:, :2] = rng.uniform(-1.3, 2.7, (P.shape[0], 2))
    I = np.arange(P.shape[0], dtype=np.uint32).reshape(-1, 3)
    M = np.asarray(kinds, np.uint32)
    lights = [_light(a, a.LIGHT_POINT, (50.0, 50.0, 50.0), (0.0, -1.0, 0.0), (100.0, 100.0, 100.0) if with_point_light else (0.0, 0.0, 0.0))]
    return DescArrays(a, P, Nn, T, I, M, mats, [(tex, True)], lights)


# ---- the area-light entry points of the oracle (typed in oracle_binding.load_oracle)
def oracle_exclude(lib, scene, tris):
    t = np.ascontiguousarray(tris, np.uint32)
    assert lib.oracle_area_exclude(scene, t.ctypes.data if len(t) else None, len(t)) == 0


def oracle_info(pkg, lib, scene):
    info = pkg.abi.AreaLightInfo()
    lib.oracle_area_light_info(scene, C.byref(info))
    return info


def oracle_table(lib, scene):
    """(prim, weight, area, cdf) of the oracle's emitter table"""
    n = int(lib.oracle_area_table(scene, None, None, None, None))
    prim = np.zeros(n, np.uint32)
    w, ar, cdf = (np.zeros(n, np.float32) for _ in range(3))
    assert lib.oracle_area_table(scene, prim.ctypes.data, w.ctypes.data, ar.ctypes.data, cdf.ctypes.data) == n
    return prim, w, ar, cdf


def oracle_sample(lib, scene, mode, states, points=None):
    states = np.ascontiguousarray(states, np.uint32).reshape(-1)
    n = states.shape[0]
    out = np.zeros((n, 16), np.float32)
    pts = None if points is None else np.ascontiguousarray(points, np.float32).reshape(n, 3)
    lib.oracle_area_light_sample(scene, mode, states.ctypes.data, None if pts is None else pts.ctypes.data, n, out.ctypes.data)
    return out


LCG_INV = 4276115653  # 1664525^-1 mod 2^32


def states_for_top_draw(count, seed=0):
    """light-start states (mode 0) whose draw a is the largest value nextRand gives, 1 - 2^-24: s' = 1664525 s +
    1013904223 inverted for s' with all 24 low bits set"""
    rng = np.random.default_rng(seed)
    hi = rng.integers(0, 256, count)
    return np.array([(((int(h) << 24) | 0xFFFFFF) - 1013904223) * LCG_INV % 2 ** 32 for h in hi], np.uint32)


# NEE states (mode 1) whose draw a = nextRand(initRand(state, AREA_KEY)) is 1 - 2^-24: initRand has no inverse from its
# output alone, so these were found by an exhaustive search of the states below 2^28
NEE_TOP_DRAW_STATES = np.array([5960030, 7904094, 16400753, 70725031, 74514276, 74810977, 82526205, 102232398, 106910346,
                                118016082, 126293959, 146967452, 161446996, 178886117, 180067756, 202601877, 212151250,
                                244036247, 251583124, 259332822], np.uint32)
