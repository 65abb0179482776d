"""A float64 numpy restatement of the area-light contract (include/bdpt.h "Area lights"): the emitter list, weights, CDF
and area pdf, the point of three uniforms, and the two draw orders (light subpath start, NEE term).  Written from the
header, not from the device code; the RNG and the cosine-hemisphere sample are the existing readings of the HLSL.

Materials are anything with the fields of bdpt_material (emissive, flags, texEmissive, texBaseColor, alphaThreshold,
baseColor); textures are (H x W x 4 uint8 array, srgb flag) pairs, row 0 first."""
import math

import numpy as np

from hlsl_integrator_numpy import hm_init_rand
from hlsl_reference_math import cos_hemisphere, luminance, next_rand

AREA_KEY = 0x41524541
CHANNEL_UNUSED, CHANNEL_CONST, CHANNEL_TEXTURE = 0, 1, 2


def emissive_type(flags):
    return (int(flags) >> 9) & 7


def diffuse_type(flags):
    return (int(flags) >> 3) & 7


def alpha_mode(flags):
    return (int(flags) >> 17) & 3


def srgb_to_linear(c):
    c = np.asarray(c, np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def bilinear(tex, srgb, u, v):
    """linear filter, wrap addressing, mip 0: RGBA (rgb sRGB-decoded when srgb), alpha = byte / 255"""
    h, w = tex.shape[:2]
    x, y = u * w - 0.5, v * h - 0.5
    x0, y0 = math.floor(x), math.floor(y)
    fx, fy = x - x0, y - y0
    ix0, iy0 = int(x0) % w, int(y0) % h
    ix1, iy1 = (ix0 + 1) % w, (iy0 + 1) % h

    def texel(ix, iy):
        p = tex[iy, ix].astype(np.float64)
        rgb = srgb_to_linear(p[:3]) if srgb else p[:3] / 255.0
        return np.append(rgb, p[3] / 255.0)

    t00, t10, t01, t11 = texel(ix0, iy0), texel(ix1, iy0), texel(ix0, iy1), texel(ix1, iy1)
    top, bot = t00 + (t10 - t00) * fx, t01 + (t11 - t01) * fx
    return top + (bot - top) * fy


class AreaTable:
    def __init__(self, positions, indices, tri_material, materials, textures=(), texcoords=None, dropped=()):
        self.P = np.asarray(positions, np.float64).reshape(-1, 3)
        self.I = np.asarray(indices, np.int64).reshape(-1, 3)
        self.M = np.asarray(tri_material, np.int64).reshape(-1)
        self.mats, self.texs = materials, list(textures)
        self.UV = None if texcoords is None else np.asarray(texcoords, np.float64).reshape(-1, 3)[:, :2]
        drop = set(int(t) for t in dropped)
        prims = []
        for t in range(self.I.shape[0]):
            m = materials[self.M[t]]
            typ = emissive_type(m.flags)
            if t in drop:
                continue
            if typ == CHANNEL_TEXTURE or (typ == CHANNEL_CONST and luminance(list(m.emissive)) > 0):
                prims.append(t)
        self.prim = np.asarray(prims, np.int64)
        self.refresh(self.P)

    def refresh(self, positions):
        """weights and CDF from (new) positions"""
        self.P = np.asarray(positions, np.float64).reshape(-1, 3)
        n = len(self.prim)
        self.area, self.w = np.zeros(n), np.zeros(n)
        for i, t in enumerate(self.prim):
            p0, p1, p2 = self.P[self.I[t]]
            self.area[i] = 0.5 * np.linalg.norm(np.cross(p1 - p0, p2 - p0))
            m = self.mats[self.M[t]]
            lam = 1.0 if emissive_type(m.flags) == CHANNEL_TEXTURE else luminance(list(m.emissive))
            self.w[i] = self.area[i] * lam
        self.cdf = np.cumsum(self.w)
        self.W = float(self.cdf[-1]) if n else 0.0
        pos = np.nonzero(self.w > 0)[0]
        self.last = int(pos[-1]) if len(pos) else -1

    def pick(self, a):
        i = int(np.searchsorted(self.cdf, a * self.W, side="right"))  # first CDF value > a W
        return i if i < len(self.prim) else self.last

    def pdf_area(self, i):
        return self.w[i] / (self.W * self.area[i])

    def _uv(self, t, b1, b2):
        if self.UV is None:
            return 0.0, 0.0
        uv = self.UV[self.I[t]]
        r = uv[0] * (1.0 - b1 - b2) + uv[1] * b1 + uv[2] * b2
        return float(r[0]), float(r[1])

    def alpha(self, t, b1, b2):
        """(alpha, threshold) of an alpha-masked triangle's material at the point, None for an opaque one"""
        m = self.mats[self.M[t]]
        if alpha_mode(m.flags) == 0:
            return None
        typ = diffuse_type(m.flags)
        if typ == CHANNEL_UNUSED:
            a = 0.0
        elif typ == CHANNEL_TEXTURE and m.texBaseColor >= 0:
            tex, srgb = self.texs[m.texBaseColor]
            a = float(bilinear(tex, srgb, *self._uv(t, b1, b2))[3])
        else:
            a = float(m.baseColor[3])
        return a, float(m.alphaThreshold)

    def emission(self, t, b1, b2):
        m = self.mats[self.M[t]]
        if emissive_type(m.flags) == CHANNEL_TEXTURE and m.texEmissive >= 0:
            tex, srgb = self.texs[m.texEmissive]
            return bilinear(tex, srgb, *self._uv(t, b1, b2))[:3]
        return np.asarray(list(m.emissive), np.float64)

    def point(self, a, u1, u2):
        """dict: emitter index, prim, barycentrics, position, n_g, Le, p_A, alpha (None or (alpha, threshold))"""
        i = self.pick(a)
        t = int(self.prim[i])
        su = math.sqrt(u1)
        b1, b2 = u2 * su, 1.0 - su
        p0, p1, p2 = self.P[self.I[t]]
        pos = p0 * (1.0 - b1 - b2) + p1 * b1 + p2 * b2
        c = np.cross(p1 - p0, p2 - p0)
        ln = np.linalg.norm(c)
        ng = c / ln if ln > 0 else np.zeros(3)
        Le = self.emission(t, b1, b2)
        al = self.alpha(t, b1, b2)
        if ln == 0 or (al is not None and al[0] < al[1]):
            Le = np.zeros(3)
        return dict(i=i, prim=t, b1=b1, b2=b2, pos=pos, ng=ng, Le=Le, pA=self.pdf_area(i), alpha=al)

    def light_start(self, state):
        """init_paths after the selection draw picked the table: (point, side normal, direction, colour, seedL)"""
        state, a = next_rand(state)
        state, u1 = next_rand(state)
        state, u2 = next_rand(state)
        state, s = next_rand(state)
        x = self.point(a, u1, u2)
        n = x["ng"] if s < 0.5 else -x["ng"]
        state, d = cos_hemisphere(state, n)
        color = x["Le"] * (2.0 * math.pi / x["pA"])
        return x, n, d, color, state

    def nee(self, state, pos):
        """a NEE term that drew the table (state: after its draw): (point, L, d, intensity)"""
        s = hm_init_rand(state, AREA_KEY)
        s, a = next_rand(s)
        s, u1 = next_rand(s)
        s, u2 = next_rand(s)
        x = self.point(a, u1, u2)
        v = x["pos"] - np.asarray(pos, np.float64)
        d2 = float(v @ v)
        if d2 == 0:
            return x, np.zeros(3), 0.0, np.zeros(3)
        d = math.sqrt(d2)
        L = v / d
        inten = x["Le"] * (abs(float(x["ng"] @ L)) / (x["pA"] * d2))
        if not np.isfinite(inten).all():
            inten = np.zeros(3)
        return x, L, d, inten
