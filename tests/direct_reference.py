"""Yardsticks of the direct lighting query (bdpt_direct_query, include/bdpt.h "Direct lighting"), none of them the code under
test.

direct_compose is the query's definition written once in numpy float32, one operation per rounding, over a small backend:
light_ray(k, rec) -> (ray, L, dist), intensity(k, rec) and any_hit(rays).  OracleBackend takes L and dist from
oracle_light_nee called on the one-light slice lights[k:k+1] (with one light the draw always picks it), visibility from
oracle_trace mode 2, and I — which no oracle hook exposes — from light_intensity, a numpy-float32 restatement of the oracle's
getLightData (its det_acos polynomial and its normalize included) that tests/test_direct_cpu.py pins against
oracle_light_nee's value bit for bit.  tests/test_gpu_direct.py answers the same backend with the existing device queries:
the composed loop.

direct_f64 is a float64 reading written from lambertianPlusShadows.rt.hlsl, LambertianPlusShadowPass.cpp and Falcor's
Lights.slang (hlsl_light_connect_math.light_data has the light part), with brute-force Moeller-Trumbore for visibility; it
reports the items it cannot arbitrate.  Plus the scenes."""
import ctypes as C

import numpy as np

import ao_reference as ar
import gi_reference as gr
import hlsl_light_connect_math as lm
from edge_rays import F64_TOL
from gi_reference import dot3, same_bits, saturate  # noqa: F401  (same_bits: for the tests)

F = np.float32
U = np.uint32
KPI = F(3.14159265358979323846)
SHADER_PI = F(3.141592)  # lambertianPlusShadows.rt.hlsl:144: the shader's literal, not M_PI
FALLBACK = F(0.00001)    # .hlsl:110
USE_HINTS = 1
LIGHT_DIRECTIONAL = 1
MAX_LIGHTS = 16


# ---- the intensity restatement -----------------------------------------------------------------------------------------
def _length(v):
    return np.sqrt(dot3(v, v))


def _normalize(v):
    inv = F(1.0) / np.sqrt(dot3(v, v))
    return (v * inv[:, None]).astype(F)


def det_acos(x):
    """the oracle's acos stand-in (Abramowitz & Stegun 4.4.46), Horner in float32"""
    x = np.asarray(x, F)
    ax = np.abs(x)
    ax = np.where(ax > F(1.0), F(1.0), ax).astype(F)
    p = np.full(ax.shape, F(-0.0012624911), F)
    for c in (0.0066700901, -0.0170881256, 0.0308918810, -0.0501743046, 0.0889789874, -0.2145988016, 1.5707963050):
        p = F(c) + ax * p
    r = np.sqrt(F(1.0) - ax) * p
    return np.where(x < 0, KPI - r, r).astype(F)


def light_intensity(lt, pos):
    """getLightData of one abi.Light at `pos` (n, 3) in numpy float32 -> (L (n, 3), I (n, 3), dist (n,))"""
    pos = np.ascontiguousarray(pos, F)
    n = len(pos)
    lpos, ldir, lint = (np.array([v[j] for j in range(3)], F) for v in (lt.posW, lt.dirW, lt.intensity))
    with np.errstate(all="ignore"):
        if lt.type == LIGHT_DIRECTIONAL:
            ls_l = np.tile(np.negative(_normalize(ldir[None])), (n, 1))
            d0 = _length(pos - lpos[None])
            ls_pos = pos - ldir[None] * d0[:, None]
            inten = np.tile(lint[None], (n, 1))
        else:
            ls_l = lpos[None] - pos
            d2 = dot3(ls_l, ls_l)
            ls_l = np.where((d2 > F(1e-5))[:, None], _normalize(ls_l), F(0)).astype(F)
            falloff = F(1.0) / ((F(0.01) * F(0.01)) + d2)
            cos_t = np.negative(dot3(ls_l, np.tile(ldir[None], (n, 1))))
            outside = cos_t < F(lt.cosOpeningAngle)
            if F(lt.penumbraAngle) > 0:
                delta = F(lt.openingAngle) - det_acos(cos_t)
                falloff = np.where(outside, falloff, falloff * saturate((delta - F(lt.penumbraAngle)) / F(lt.penumbraAngle)))
            falloff = np.where(outside, F(0), falloff).astype(F)
            ls_pos = np.tile(lpos[None], (n, 1))
            inten = lint[None] * falloff[:, None]
        return _normalize(ls_l), inten.astype(F), _length(ls_pos - pos).astype(F)


# ---- the definition ----------------------------------------------------------------------------------------------------
def albedo(rec):
    """dif, or specular where dot(dif, dif) < 0.00001 (.hlsl:109-114)"""
    dif, spec = rec[:, 12:15], rec[:, 16:19]
    with np.errstate(all="ignore"):
        return np.where((dot3(dif, dif) < FALLBACK)[:, None], spec, dif).astype(F)


def direct_compose(q, rec, min_t, alive=None, trace_all=False):
    """bdpt_direct_query's definition over backend `q` on (n, 24) bdpt_surface records.  trace_all: ask any_hit for every
    live (item, light) pair, the rays that cannot change the result included (the no-ray rule's test).
    -> dict(color (n, 4) float32, visible (n,) uint32, traced (n,) uint32, live (n,) bool, and per light rays [(n, 8)],
    need [(n,) bool], ldn [(n,)], inten [(n, 3)])"""
    rec = np.ascontiguousarray(rec, F)
    n = len(rec)
    live = rec.view(np.int32)[:, 23] >= 0
    if alive is not None:
        live = live & (np.asarray(alive) != 0)
    nrm = rec[:, 4:7]
    dif = albedo(rec)
    total = np.zeros((n, 3), F)
    visible, traced = np.zeros(n, U), np.zeros(n, U)
    out = dict(rays=[], need=[], ldn=[], inten=[])
    with np.errstate(all="ignore"):
        for k in range(q.num_lights):
            ray, L, _ = q.light_ray(k, rec)
            inten = q.intensity(k, rec)
            ldn = saturate(dot3(nrm, L))
            need = live & (ldn != 0) & ~(inten == 0).all(axis=1)
            ask = live if trace_all else need
            vis = np.ones(n, bool)
            if ask.any():
                vis[ask] = q.any_hit(ray[ask])
            s = np.where(ask & ~vis, F(0), F(1)).astype(F)
            total = total + (s * ldn)[:, None] * inten
            visible |= (s != 0).astype(U) << U(k)
            traced |= need.astype(U) << U(k)
            out["rays"].append(ray), out["need"].append(need), out["ldn"].append(ldn), out["inten"].append(inten)
        color = total * (dif / SHADER_PI)
    color = np.concatenate([np.where(live[:, None], color, dif), np.ones((n, 1), F)], axis=1).astype(F)
    out.update(color=color, visible=np.where(live, visible, 0).astype(U), traced=np.where(live, traced, 0).astype(U), live=live)
    return out


def one_light(abi, lights, k):
    """the one-light table lights[k:k+1]"""
    arr = (abi.Light * 1)()
    C.memmove(arr, C.byref(lights[k]), C.sizeof(abi.Light))
    return arr


class OracleBackend:
    """direct_compose's backend from the CPU oracle's hooks and the pinned restatement"""

    def __init__(self, ob, abi, lib, osc, lights, min_t):
        self.ob, self.abi, self.lib, self.osc, self.lights, self.min_t = ob, abi, lib, osc, lights, min_t
        self.num_lights = len(lights)

    def light_ray(self, k, rec):
        smp, _ = self.ob.light_nee(self.abi, one_light(self.abi, self.lights, k), rec, np.zeros(len(rec), U), 1, self.min_t)
        return smp[:, 0:8].copy(), smp[:, 4:7].copy(), smp[:, 7].copy()

    def intensity(self, k, rec):
        return light_intensity(self.lights[k], rec[:, 0:3])[1]

    def any_hit(self, rays):
        m = len(rays)
        r = np.zeros((m, 8), F)  # oracle_trace's layout: origin, direction, tmin, tmax
        r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7] = rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7]
        prim, tuv = np.zeros(m, np.int32), np.zeros((m, 3), F)
        self.lib.oracle_trace(self.osc, r.ctypes.data, m, 2, 0, prim.ctypes.data, tuv.ctypes.data)
        return prim < 0


def direct_oracle(ob, abi, lib, osc, lights, rec, min_t, **kw):
    return direct_compose(OracleBackend(ob, abi, lib, osc, lights, min_t), rec, min_t, **kw)


def pin_value(ldn, inten):
    """(((1 * LdotN) * I) * 1) / kPi: what oracle_light_nee's value is for one light and diffuse = (1, 1, 1)"""
    with np.errstate(all="ignore"):
        return ((((F(1) * ldn)[:, None] * inten) * F(1)) / KPI).astype(F)


# ---- scenes ------------------------------------------------------------------------------------------------------------
def sixteen_lights(abi):
    """16 lights inside the unit room: point lights, spot lights with and without a penumbra, directional lights"""
    rng = np.random.default_rng(16)
    lights = (abi.Light * MAX_LIGHTS)()
    for k in range(MAX_LIGHTS):
        lt = lights[k]
        kind = k % 4  # point, spot with a penumbra, directional, spot without
        d = rng.normal(size=3)
        d[1] = -abs(d[1]) - 0.5  # downward
        d = d / np.linalg.norm(d)
        for j in range(3):
            lt.posW[j] = float(F(rng.uniform(-0.8, 0.8) if j != 1 else rng.uniform(0.3, 0.9)))
            lt.dirW[j] = float(F(d[j]))
            lt.intensity[j] = float(F(rng.uniform(0.2, 1.5)))
        if kind == 2:
            lt.type = abi.LIGHT_DIRECTIONAL
        else:
            lt.type = abi.LIGHT_POINT
            opening = np.pi if kind == 0 else rng.uniform(0.6, 1.2)
            lt.openingAngle, lt.cosOpeningAngle = float(F(opening)), float(F(np.cos(np.float64(F(opening))))) if kind else -1.0
            lt.penumbraAngle = float(F(rng.uniform(0.1, 0.3))) if kind == 1 else 0.0
    return lights


class DirectScene(ar.QuadScene):
    """ao_reference's room with blocks under a light table: None = QuadScene's one point light"""

    def __init__(self, pkg, lights=None):
        super().__init__(pkg, ar.room_quads())
        if lights is None:
            lights = one_light(pkg.abi, self.desc.lights, 0)  # at (0, 0.9, 0); made a whole sphere: a zero dirW sits on the cone's edge
            lights[0].openingAngle, lights[0].cosOpeningAngle = float(F(np.pi)), -1.0
        self.lights = lights
        self.desc.lights, self.desc.numLights = lights, len(lights)
        self.keep.append(lights)

    def records(self, rng, n, misses=0, dead_run=None):
        """n surface points as bdpt_surface records with diffuse and specular colours (every seventh diffuse black or nearly:
        the fallback), `misses` miss records appended, and with dead_run = (start, length) a stretch of miss records"""
        pos, nrm = self.surface_points(rng, n)
        rec = ar.surface_records(pos, nrm)
        rec[:, 12:15] = rng.uniform(0.1, 0.9, (n, 3)).astype(F)
        rec[:, 16:19] = rng.uniform(0.1, 0.9, (n, 3)).astype(F)
        rec[::7, 12:15] = rng.choice(np.array([0.0, 1e-3, 1.8e-3, 1.9e-3, 4e-3], F), size=(len(rec[::7]), 1))  # 3 * 0.0018^2 < 1e-5 < 3 * 0.0019^2
        if misses:
            miss = rng.uniform(-1, 1, (misses, 24)).astype(F)
            miss[:, 12:15] = np.abs(miss[:, 12:15]) * F(np.arange(misses) % 2)[:, None]  # every other one black: the fallback of a dead item
            miss.view(np.int32)[:, 23] = -1 - np.arange(misses, dtype=np.int32) % 3
            rec = np.concatenate([rec, miss])
        if dead_run:
            a, m = dead_run
            rec.view(np.int32)[a:a + m, 23] = -1
        return rec


def three_light_scene(pkg):
    return DirectScene(pkg, gr.three_lights(pkg.abi))


def sixteen_light_scene(pkg):
    return DirectScene(pkg, sixteen_lights(pkg.abi))


# ---- the float64 reading -------------------------------------------------------------------------------------------------
CONE_TOL, FALLBACK_TOL = 1e-6, 1e-7


def _light_dict(lt):
    return dict(type=int(lt.type), posW=[lt.posW[j] for j in range(3)], dirW=[lt.dirW[j] for j in range(3)],
                intensity=[lt.intensity[j] for j in range(3)], openingAngle=float(lt.openingAngle),
                cosOpeningAngle=float(lt.cosOpeningAngle), penumbraAngle=float(lt.penumbraAngle))


def _f64_occluded(sc, org, seg, tmin):
    """any hit of the segments org + t * seg, t in (tmin, 1) (tmin per ray) -> (occluded, near an edge or an interval end)"""
    p = np.asarray(sc.pos, np.float64)
    v0 = p[sc.tri[:, 0]]
    e1, e2 = p[sc.tri[:, 1]] - v0, p[sc.tri[:, 2]] - v0
    occ, left = np.zeros(len(org), bool), np.zeros(len(org), bool)
    for a in range(0, len(org), 1024):
        oo, dd, tm = org[a:a + 1024][:, None], seg[a:a + 1024][:, None], tmin[a:a + 1024][:, None]
        with np.errstate(all="ignore"):
            pv = np.cross(dd, e2[None])
            det = (e1[None] * pv).sum(-1)
            inv = 1.0 / det
            tv = oo - v0[None]
            u = (tv * pv).sum(-1) * inv
            qv = np.cross(tv, e1[None])
            v = (dd * qv).sum(-1) * inv
            t = (e2[None] * qv).sum(-1) * inv
            margin = np.minimum(np.minimum(u, v), 1.0 - u - v)
            ok = (det != 0) & np.isfinite(t) & np.isfinite(margin)
            hit = ok & (margin >= 0) & (t > tm) & (t < 1.0)
            cand = ok & (margin > -F64_TOL) & (t > tm - F64_TOL * tm) & (t < 1.0 + F64_TOL)
            near = cand & ((np.abs(margin) < F64_TOL) | (np.abs(t - tm) <= F64_TOL * np.abs(t)) | (np.abs(t - 1.0) <= F64_TOL * np.abs(t)))
        occ[a:a + 1024], left[a:a + 1024] = hit.any(axis=1), near.any(axis=1)
    return occ, left


def direct_f64(sc, rec, min_t):
    """the shader on DirectScene `sc` -> dict(color (n, 3) float64, left_out: {cause: (n,) bool}, live)"""
    rec = np.asarray(rec, F)
    n = len(rec)
    live = rec.view(np.int32)[:, 23] >= 0
    pos, nrm, dif, spec = (rec[:, c].astype(np.float64) for c in (slice(0, 3), slice(4, 7), slice(12, 15), slice(16, 19)))
    dd = (dif * dif).sum(axis=1)
    fallback_amb = np.abs(dd - 0.00001) < FALLBACK_TOL
    dif = np.where((dd < 0.00001)[:, None], spec, dif)
    edge, cone = np.zeros(n, bool), np.zeros(n, bool)
    total = np.zeros((n, 3))
    tmin = float(F(min_t))
    for k in range(len(sc.lights)):
        lt = _light_dict(sc.lights[k])
        L, inten, dist = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
        for i in np.nonzero(live)[0]:
            L[i], inten[i], dist[i], m = lm.light_data(lt, pos[i])
            cone[i] |= lt["type"] != LIGHT_DIRECTIONAL and min(m["cone"], m["acos_domain"]) < CONE_TOL
        with np.errstate(all="ignore"):
            ldn = np.clip((nrm * L).sum(axis=1), 0.0, 1.0)
            ldn = np.where(np.isnan(ldn), 0.0, ldn)
            term = ldn[:, None] * inten
            idx = np.nonzero(live & (term != 0).any(axis=1))[0]
            shadow = np.ones(n)
            if len(idx):
                occ, near = _f64_occluded(sc, pos[idx], L[idx] * dist[idx, None], tmin / dist[idx])
                shadow[idx] = np.where(occ, 0.0, 1.0)
                edge[idx] |= near
            total += shadow[:, None] * term
    with np.errstate(all="ignore"):
        color = total * (dif / 3.141592)
    color = np.where(live[:, None], color, dif)
    left = dict(edge=edge & live, cone=cone & live, fallback=fallback_amb)
    return dict(color=color, left_out=left, live=live)
