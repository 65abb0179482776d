"""Yardsticks of the diffuse GI query (bdpt_gi_query, include/bdpt.h "Diffuse GI"), none of them the code under test.

gi_compose is the query's definition written once over a small backend interface (a NEE term, an any-hit trace, a closest-hit
trace, the cosine direction, hit shading); OracleBackend answers it with the CPU oracle's hooks (oracle_light_nee with matIndex
1, oracle_trace in modes 2 and 0, oracle_bsdf with matIndex 1, oracle_shade_hits) and that is gi_oracle; tests/test_gpu_gi.py
answers it with the existing device queries and that is the composed loop.  The LCG runs in exact uint32 numpy, and the final
arithmetic in numpy float32, one operation per rounding.  The uniform direction is a numpy-float32 restatement whose shared
part is pinned through its cosine variant (test_gi_cpu.py).  The environment map's texel comes from a float64 atan2 / acos;
items whose u * W or v * H lies within ENV_TOL of an integer are reported as ambiguous.  Plus the scenes."""
import numpy as np

import ao_reference as ar
from ao_reference import lcg

F = np.float32
U = np.uint32
KPI = F(3.14159265358979323846)
INDIRECT, UNIFORM, FROM_VIEW = 1, 2, 4
DIRECT_OCCLUDED, BOUNCE_HIT, BOUNCE_OCCLUDED = 1, 2, 4
NORMAL_MAP = 1
ENV_TOL = 1e-4


def rand_float(s):
    """nextRand's float of the state after the draw"""
    return (np.asarray(s, U) & U(0x00FFFFFF)).astype(F) / F(16777216.0)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def saturate(x):
    """HLSL saturate: NaN gives 0"""
    with np.errstate(invalid="ignore"):
        y = np.where(x > 0, x, F(0))
        return np.where(y < 1, y, F(1)).astype(F)


def hemisphere_direction(lib, seeds, nrm, uniform):
    """getCosHemisphereSample / getUniformHemisphereSample (simpleDiffuseGIUtils.hlsli:114-143) in numpy float32, the sine and
    cosine from oracle_sincos2pi: two draws from `seeds` -> (directions (n, 3) float32, the states after)"""
    nrm = np.ascontiguousarray(nrm, F)
    s1 = lcg(seeds)
    s2 = lcg(s1)
    r0, r1 = rand_float(s1), np.ascontiguousarray(rand_float(s2))
    with np.errstate(all="ignore"):
        a = np.abs(nrm)
        xm = ((a[:, 0] - a[:, 1]) < 0) & ((a[:, 0] - a[:, 2]) < 0)
        ym = ((a[:, 1] - a[:, 2]) < 0) & ~xm
        zm = ~(xm | ym)
        bitangent = _cross(nrm, np.stack([xm, ym, zm], axis=1).astype(F))
        tangent = _cross(bitangent, nrm)
        if uniform:
            x = F(1) - r0 * r0
            r, z = np.sqrt(np.where(x > 0, x, F(0)).astype(F)), r0
        else:
            x = F(1) - r0
            r, z = np.sqrt(r0), np.sqrt(np.where(x > 0, x, F(0)).astype(F))
        sn, cs = np.zeros(len(r1), F), np.zeros(len(r1), F)
        lib.oracle_sincos2pi(r1.ctypes.data, len(r1), sn.ctypes.data, cs.ctypes.data)
        d = (tangent * (r * cs)[:, None] + bitangent * (r * sn)[:, None]) + nrm * z[:, None]
    return d.astype(F), s2


def env_lookup(dirs, env):
    """IndirectMiss: env None -> black, four floats -> that colour, an (H, W, 4) float32 map -> its lat-long texel, looked up
    in float64 -> (colours (n, 3) float32, ambiguous (n,) bool)"""
    n = len(dirs)
    if env is None:
        return np.zeros((n, 3), F), np.zeros(n, bool)
    env = np.asarray(env, F)
    if env.ndim == 1:
        return np.tile(env[None, 0:3], (n, 1)), np.zeros(n, bool)
    h, w = env.shape[0:2]
    d = np.asarray(dirs, np.float64)
    with np.errstate(all="ignore"):
        pd = d / np.sqrt((d * d).sum(axis=1))[:, None]
        u = (1.0 + np.arctan2(pd[:, 0], -pd[:, 2]) / np.pi) * 0.5 * w
        v = np.arccos(np.clip(pd[:, 1], -1.0, 1.0)) / np.pi * h
        bad = ~np.isfinite(u) | ~np.isfinite(v)
        u, v = np.where(bad, 0.0, u), np.where(bad, 0.0, v)
        amb = bad | (np.abs(u - np.round(u)) < ENV_TOL) | (np.abs(v - np.round(v)) < ENV_TOL)
        ex, ey = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    inside = (ex >= 0) & (ex < w) & (ey >= 0) & (ey < h)
    col = np.where(inside[:, None], env[np.clip(ey, 0, h - 1), np.clip(ex, 0, w - 1), 0:3], F(0))
    return col.astype(F), amb


def gi_compose(q, rec, seeds, flags, min_t, view_pos=None, shade_flags=0, env=None, alive=None):
    """bdpt_gi_query's definition over backend `q` on (n, 24) bdpt_surface records.
    -> dict(color (n, 4) float32, hits (n, 4) float32, status (n,) uint32, seeds_out (n,) uint32, live (n,) bool, and for
    the float64 reading and the tests: light1 / light2 (n,) the lights chosen, ray1 / ray2 (n, 8) the shadow rays, traced1 /
    traced2 (n,) bool, dirs (n, 3), rec2 (n, 24) the shaded bounce hits, env_ambiguous (n,) bool)"""
    rec = np.ascontiguousarray(rec, F)
    n = len(rec)
    s0 = np.ascontiguousarray(seeds, U)
    live = rec.view(np.int32)[:, 23] >= 0
    if alive is not None:
        live = live & (np.asarray(alive) != 0)
    indirect, uniform = bool(flags & INDIRECT), bool(flags & UNIFORM)
    pos, nrm, dif = rec[:, 0:3], rec[:, 4:7], rec[:, 12:15]
    zero3 = np.zeros((n, 3), F)

    def term(smp, vis):
        word = smp.view(U)[:, 11]
        traced = ((word >> 16) & 1) != 0
        value = np.where((traced & ~vis)[:, None], zero3, smp[:, 8:11])  # occluded: exactly +0
        return value, traced, traced & ~vis, (word & 0xFFFF)

    with np.errstate(all="ignore"):
        smp1, s1 = q.nee(rec, s0)
        direct, traced1, occ1, light1 = term(smp1, q.any_hit(smp1[:, 0:8]))
        status = np.where(occ1, DIRECT_OCCLUDED, 0).astype(U)
        color = direct.copy()
        hits = np.zeros((n, 4), F)
        hits.view(np.int32)[:, 3] = -1
        out = dict(light1=light1, ray1=smp1[:, 0:8].copy(), traced1=traced1, dirs=zero3.copy(), rec2=np.zeros((n, 24), F),
                   ray2=np.zeros((n, 8), F), traced2=np.zeros(n, bool), light2=np.zeros(n, U), env_ambiguous=np.zeros(n, bool))
        s_out = s1
        if indirect:
            if uniform:
                dirs, s3 = hemisphere_direction(q.lib, s1, nrm, True)
            else:
                dirs, s3 = q.cosine_direction(rec, s1), lcg(lcg(s1))
            s_out = s3
            ndl = saturate(dot3(nrm, dirs))
            rays = np.zeros((n, 8), F)
            rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = pos, F(min_t), dirs, F(1e38)
            h = q.closest_hit(rays)
            hit = h.view(np.int32)[:, 3] >= 0
            hits = np.where(hit[:, None], h, hits)
            from_rays = rays.copy()
            if flags & FROM_VIEW:
                from_rays[:, 0:3] = np.asarray(view_pos, F)
            rec2 = q.shade(from_rays, hits, shade_flags)
            smp2, _ = q.nee(rec2, s3)  # t = s, a copy: the item's own state does not advance
            b_hit, traced2, occ2, light2 = term(smp2, q.any_hit(smp2[:, 0:8]))
            b_env, amb = env_lookup(dirs, env)
            bounce = np.where(hit[:, None], b_hit, b_env)
            status |= np.where(hit, BOUNCE_HIT, 0).astype(U) | np.where(hit & occ2, BOUNCE_OCCLUDED, 0).astype(U)
            prob = np.full(n, F(1) / (F(2) * KPI), F) if uniform else ndl / KPI
            color = direct + (((ndl[:, None] * bounce) * dif) / KPI) / prob[:, None]
            out.update(dirs=dirs, rec2=rec2, ray2=smp2[:, 0:8].copy(), traced2=traced2 & hit, light2=light2, env_ambiguous=amb & ~hit & live)
    color = np.concatenate([np.where(live[:, None], color, dif), np.ones((n, 1), F)], axis=1).astype(F)
    hits = np.where(live[:, None], hits, F(0))
    hits.view(np.int32)[~live, 3] = -1
    out.update(color=color, hits=hits, status=np.where(live, status, 0).astype(U), seeds_out=np.where(live, s_out, s0).astype(U), live=live)
    return out


class OracleBackend:
    """gi_compose's backend from the CPU oracle's hooks"""

    def __init__(self, ob, abi, lib, osc, lights, min_t):
        self.ob, self.abi, self.lib, self.osc, self.lights, self.min_t = ob, abi, lib, osc, lights, min_t

    def nee(self, rec, seeds):
        return self.ob.light_nee(self.abi, self.lights, rec, seeds, 1, self.min_t)

    def _trace(self, rays, mode):
        m = len(rays)
        r = np.zeros((m, 8), F)  # oracle_trace's layout: origin, direction, tmin, tmax
        r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7] = rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7]
        prim, tuv = np.zeros(m, np.int32), np.zeros((m, 3), F)
        self.lib.oracle_trace(self.osc, r.ctypes.data, m, mode, 0, prim.ctypes.data, tuv.ctypes.data)
        return prim, tuv

    def any_hit(self, rays):
        return self._trace(rays, 2)[0] < 0  # visible

    def closest_hit(self, rays):
        prim, tuv = self._trace(rays, 0)
        h = np.zeros((len(rays), 4), F)
        h[:, 0:3] = np.where((prim >= 0)[:, None], tuv, F(0))
        h.view(np.int32)[:, 3] = prim
        return h

    def cosine_direction(self, rec, seeds):
        m = len(rec)
        bs_in, bs_out = np.zeros((m, 20), F), np.zeros((m, 16), F)
        bs_in[:, 0:3] = rec[:, 4:7]
        bs_in.view(U)[:, 17] = seeds
        self.lib.oracle_bsdf(bs_in.ctypes.data, m, 1, bs_out.ctypes.data)
        return bs_out[:, 3:6].copy()

    def shade(self, rays, hits, flags):
        return self.ob.shade_hits(self.abi, self.osc, rays, hits, flags)


def gi_oracle(ob, abi, lib, osc, lights, rec, seeds, flags, min_t, **kw):
    return gi_compose(OracleBackend(ob, abi, lib, osc, lights, min_t), rec, seeds, flags, min_t, **kw)


# ---- scenes ------------------------------------------------------------------------------------------------------------
def three_lights(abi):
    """a point light, a spot light with a penumbra and a directional light, inside the unit room"""
    lights = (abi.Light * 3)()
    p, s, d = lights[0], lights[1], lights[2]
    p.type = abi.LIGHT_POINT
    p.posW[0], p.posW[1], p.posW[2] = 0.1, 0.85, 0.2
    p.openingAngle, p.cosOpeningAngle = float(F(np.pi)), -1.0
    p.intensity[0], p.intensity[1], p.intensity[2] = 1.0, 0.9, 0.8
    s.type = abi.LIGHT_POINT
    s.posW[0], s.posW[1], s.posW[2] = -0.6, 0.8, 0.7
    s.dirW[0], s.dirW[1], s.dirW[2] = [float(F(x)) for x in np.array([0.5, -0.8, -0.33]) / np.linalg.norm([0.5, -0.8, -0.33])]
    s.openingAngle, s.cosOpeningAngle, s.penumbraAngle = float(F(0.9)), float(F(np.cos(0.9))), float(F(0.2))
    s.intensity[0], s.intensity[1], s.intensity[2] = 0.7, 1.2, 0.6
    d.type = abi.LIGHT_DIRECTIONAL
    d.dirW[0], d.dirW[1], d.dirW[2] = [float(F(x)) for x in np.array([-0.3, -0.9, -0.3]) / np.linalg.norm([-0.3, -0.9, -0.3])]
    d.intensity[0], d.intensity[1], d.intensity[2] = 0.4, 0.4, 0.5
    return lights


class RoomScene(ar.QuadScene):
    """ao_reference's room with blocks (or the room open at the top: no ceiling, no blocks) under three_lights"""

    def __init__(self, pkg, open_top=False):
        quads = ar.room_quads(blocks=not open_top)
        if open_top:
            del quads[1]  # the ceiling
        super().__init__(pkg, quads)
        self.lights = three_lights(pkg.abi)
        self.desc.lights, self.desc.numLights = self.lights, 3
        self.keep.append(self.lights)

    def records(self, rng, n, misses=0):
        """n surface points as bdpt_surface records with a diffuse colour each, `misses` miss records appended, and seeds"""
        pos, nrm = self.surface_points(rng, n)
        rec = ar.surface_records(pos, nrm)
        rec[:, 12:15] = rng.uniform(0.1, 0.9, (n, 3)).astype(F)
        if misses:
            miss = rng.uniform(-1, 1, (misses, 24)).astype(F)
            miss.view(np.int32)[:, 23] = -1 - np.arange(misses, dtype=np.int32) % 3
            rec = np.concatenate([rec, miss])
        seeds = rng.integers(0, 2**32, len(rec), dtype=np.uint64).astype(U)
        return rec, seeds


def env_map_8x4():
    """an 8 x 4 RGBA32F map of distinct texels"""
    k = np.arange(32, dtype=F).reshape(4, 8)
    return np.stack([F(0.1) + k / F(40), F(0.9) - k / F(50), F(0.3) + (k % 5) / F(10), np.ones_like(k)], axis=2).astype(F)


def same_bits(got, want):
    """element-wise: equal as integers, or both NaN (0 / 0 is a NaN of either sign, by the machine that divides)"""
    g, w = np.asarray(got), np.asarray(want)
    if g.dtype.kind != "f":
        return g.view(U) == w.view(U)
    return (g.view(U) == w.view(U)) | (np.isnan(g) & np.isnan(w))


# ---- the float64 reading -------------------------------------------------------------------------------------------------
# Written from simpleDiffuseGI.rt.hlsl and simpleDiffuseGIUtils.hlsli (and Falcor's Lights.slang for getLightData), in float64
# with the true sin / cos / acos, for scenes of QuadScene's kind: one constant, double-sided, opaque material.
def _unit(v):
    with np.errstate(all="ignore"):
        return v / np.sqrt((v * v).sum(axis=-1))[..., None]


def _f64_rand(s):
    return (np.asarray(s, U) & U(0x00FFFFFF)).astype(np.float64) / 16777216.0


def f64_hemisphere(seeds, nrm, uniform):
    """the two hemisphere samplers (simpleDiffuseGIUtils.hlsli:114-143) -> (directions (n, 3) float64, states after)"""
    s1 = lcg(seeds)
    s2 = lcg(s1)
    r0, r1 = _f64_rand(s1), _f64_rand(s2)
    nrm = np.asarray(nrm, np.float64)
    bitangent = ar._perpendicular(nrm)
    tangent = np.cross(bitangent, nrm)
    phi = 2.0 * np.pi * r1
    r, z = (np.sqrt(np.maximum(0.0, 1.0 - r0 * r0)), r0) if uniform else (np.sqrt(r0), np.sqrt(np.maximum(0.0, 1.0 - r0)))
    return tangent * (r * np.cos(phi))[:, None] + bitangent * (r * np.sin(phi))[:, None] + nrm * z[:, None], s2


def f64_light_term(lights, seeds, pos, nrm, dif):
    """a random light, getLightData and the Lambertian term of a VISIBLE light (.hlsl:92-107, 155-170) ->
    (value (n, 3), L (n, 3), distance (n,), light (n,), ambiguous (n,): r * lightsCount within 1e-6 of an integer, states after)"""
    n_l = len(lights)
    s1 = lcg(seeds)
    x = _f64_rand(s1) * n_l
    light = np.minimum(np.floor(x).astype(np.int64), n_l - 1)
    amb = np.abs(x - np.round(x)) < 1e-6
    pos, nrm, dif = (np.asarray(a, np.float64) for a in (pos, nrm, dif))
    L, inten, dist = np.zeros_like(pos), np.zeros_like(pos), np.zeros(len(pos))
    with np.errstate(all="ignore"):
        for k in range(n_l):
            lt = lights[k]
            m = light == k
            lpos, ldir, col = (np.array([v[j] for j in range(3)], np.float64) for v in (lt.posW, lt.dirW, lt.intensity))
            p = pos[m]
            if lt.type == 1:  # directional (Lights.slang:54-66)
                d = np.sqrt(((p - lpos) ** 2).sum(axis=1))
                L[m], inten[m] = -_unit(ldir), col
                dist[m] = np.sqrt((((p - ldir * d[:, None]) - p) ** 2).sum(axis=1))
            else:  # point / spot (Lights.slang:68-102)
                to = lpos - p
                d2 = (to * to).sum(axis=1)
                unit = np.where((d2 > 1e-5)[:, None], _unit(to), 0.0)
                falloff = 1.0 / (0.01 * 0.01 + d2)
                cos_t = -(unit * ldir).sum(axis=1)
                if lt.penumbraAngle > 0:
                    delta = lt.openingAngle - np.arccos(np.clip(cos_t, -1.0, 1.0))
                    falloff = falloff * np.clip((delta - lt.penumbraAngle) / lt.penumbraAngle, 0.0, 1.0)
                falloff = np.where(cos_t < lt.cosOpeningAngle, 0.0, falloff)
                L[m], inten[m], dist[m] = _unit(unit), col * falloff[:, None], np.sqrt(d2)
        ldn = np.clip((nrm * L).sum(axis=1), 0.0, 1.0)
        ldn = np.where(np.isnan(ldn), 0.0, ldn)
        value = (n_l * ldn)[:, None] * inten * dif / np.pi
    return value, L, dist, light, amb, s1


def f64_closest_hit(pos, tri, org, dirs, tmin, tmax, chunk=1024):
    """Moeller-Trumbore in float64 over every triangle, the closest-hit rule -> (prim, t, near an edge or the interval's ends,
    runner-up within F64_TOL)"""
    from edge_rays import F64_TOL
    p = np.asarray(pos, np.float64)
    v0 = p[tri[:, 0]]
    e1, e2 = p[tri[:, 1]] - v0, p[tri[:, 2]] - v0
    n = len(org)
    prim, tt, near_any, close = np.full(n, -1, np.int64), np.zeros(n), np.zeros(n, bool), np.zeros(n, bool)
    for a in range(0, n, chunk):
        o, d = np.asarray(org[a:a + chunk], np.float64)[:, None], np.asarray(dirs[a:a + chunk], np.float64)[:, None]
        with np.errstate(all="ignore"):
            pv = np.cross(d, e2[None])
            det = (e1[None] * pv).sum(-1)
            inv = 1.0 / det
            tv = o - v0[None]
            u = (tv * pv).sum(-1) * inv
            qv = np.cross(tv, e1[None])
            v = (d * qv).sum(-1) * inv
            t = (e2[None] * qv).sum(-1) * inv
            margin = np.minimum(np.minimum(u, v), 1.0 - u - v)
            ok = (det != 0) & np.isfinite(t) & np.isfinite(margin)
            hit = ok & (margin >= 0) & (t > tmin) & (t < tmax)
            cand = ok & (margin > -F64_TOL) & (t > tmin - F64_TOL * abs(tmin)) & (t < tmax + F64_TOL * abs(tmax))
            near = cand & ((np.abs(margin) < F64_TOL) | (np.abs(t - tmin) <= F64_TOL * np.abs(t)) | (np.abs(t - tmax) <= F64_TOL * np.abs(t)))
        th = np.where(hit, t, np.inf)
        m = len(th)
        first = th.argmin(axis=1)
        t1 = th[np.arange(m), first]
        got = np.isfinite(t1)
        th[np.arange(m), first] = np.inf
        t2 = th.min(axis=1)
        # two triangles of one plane (a quad's diagonal, a box standing on the floor) answer with the same point: no runner-up
        prim[a:a + chunk], tt[a:a + chunk] = np.where(got, first, -1), np.where(got, t1, 0.0)
        near_any[a:a + chunk] = near.any(axis=1)
        close[a:a + chunk] = got & np.isfinite(t2) & (t2 - np.where(got, t1, 0.0) <= F64_TOL * np.abs(t1))
    return prim, tt, near_any, close


def gi_f64(sc, rec, seeds, flags, min_t, view_pos=None, env=None):
    """the shader pair on QuadScene `sc` (its lights: sc.lights) -> dict(color (n, 3) float64, left_out: {cause: (n,) bool})"""
    rec = np.asarray(rec, F)
    n = len(rec)
    live = rec.view(np.int32)[:, 23] >= 0
    pos, nrm, dif = (rec[:, c].astype(np.float64) for c in (slice(0, 3), slice(4, 7), slice(12, 15)))
    tmin = float(F(min_t))
    tri_n = np.repeat(np.stack([q[1] for q in sc.quads]).astype(np.float64), 2, axis=0)  # the face normal of each triangle
    mat_dif = np.array([sc.desc.materials[0].baseColor[k] for k in range(3)], np.float64)
    edge, runner, env_amb = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)

    def shadowed(value, org, L, dist):
        """term(value, ray): no ray for a value of zero, zero when the segment to the light is occluded -> (value, left out)"""
        traced = (value != 0).any(axis=1)
        occ, left = np.zeros(n, bool), np.zeros(n, bool)
        idx = np.nonzero(traced)[0]
        # (tmax differs per ray: each ray is scaled so that its interval ends at 1; ao_reference.f64_any_hit's rules otherwise)
        o, l_, t_ = org[idx], L[idx] * dist[idx, None], tmin / dist[idx]
        if len(idx):
            p = np.asarray(sc.pos, np.float64)
            v0 = p[sc.tri[:, 0]]
            e1, e2 = p[sc.tri[:, 1]] - v0, p[sc.tri[:, 2]] - v0
            from edge_rays import F64_TOL
            for a in range(0, len(idx), 1024):
                oo, dd, tm = o[a:a + 1024][:, None], l_[a:a + 1024][:, None], t_[a:a + 1024][:, None]
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
                occ[idx[a:a + 1024]], left[idx[a:a + 1024]] = hit.any(axis=1), near.any(axis=1)
        return np.where(occ[:, None], 0.0, value), left

    with np.errstate(all="ignore"):
        value1, L1, dist1, _, amb1, s1 = f64_light_term(sc.lights, seeds, pos, nrm, dif)
        direct, left1 = shadowed(value1, pos, L1, dist1)
        edge |= left1
        select = amb1.copy()
        color = direct.copy()
        if flags & INDIRECT:
            uniform = bool(flags & UNIFORM)
            dirs, s3 = f64_hemisphere(s1, nrm, uniform)
            ndl = np.clip((nrm * dirs).sum(axis=1), 0.0, 1.0)
            prim, t, near, close = f64_closest_hit(sc.pos, sc.tri, pos, dirs, tmin, 1e38)
            edge |= near
            runner |= close
            hit = prim >= 0
            hp = pos + dirs * t[:, None]
            hn = tri_n[np.maximum(prim, 0)]
            eye = np.asarray(view_pos, np.float64)[None] if flags & FROM_VIEW else pos
            hn = np.where((((eye - hp) * hn).sum(axis=1) <= 0)[:, None], -hn, hn)  # double sided: toward the view point
            value2, L2, dist2, _, amb2, _ = f64_light_term(sc.lights, s3, hp, hn, np.tile(mat_dif, (n, 1)))
            b_hit, left2 = shadowed(np.where(hit[:, None], value2, 0.0), hp, L2, dist2)
            edge |= left2 & hit
            select |= amb2 & hit
            b_env, amb = env_lookup(dirs, env)
            env_amb = amb & ~hit
            bounce = np.where(hit[:, None], b_hit, b_env.astype(np.float64))
            prob = np.full(n, 1.0 / (2.0 * np.pi)) if uniform else ndl / np.pi
            color = direct + (ndl[:, None] * bounce * dif / np.pi) / prob[:, None]
    color = np.where(live[:, None], color, dif)
    left = dict(edge=edge & live, runner_up=runner & live, light_choice=select & live, environment=env_amb & live)
    return dict(color=color, left_out=left, live=live)
