"""Yardsticks of the ambient occlusion query (bdpt_ao_query, include/bdpt.h "Ambient occlusion"), none of them the code under
test: ao_oracle composes the CPU oracle's hooks (oracle_bsdf with matIndex 1 for the directions, oracle_trace mode 2 for the
visibility) with the LCG of nextRand in exact uint32 numpy; ao_f64 is a separately written float64 reading of the reference's
shader (CommonPasses/Data/CommonPasses/aoTracing.rt.hlsl:74-122, aoCommonUtils.hlsli:21-65) with the any-hit rule only.  Plus
small numpy-built scenes."""
import ctypes as C

import numpy as np

from edge_rays import F64_TOL

F = np.float32
U = np.uint32


def lcg(s):
    """the state after one nextRand (BDPT/BDPTUtils.hlsli:103-110): exact uint32 arithmetic"""
    return (np.asarray(s, np.uint64) * np.uint64(1664525) + np.uint64(1013904223)).astype(U)


def lcg_chain(s, draws):
    """(n, draws) states: column k is the state after k + 1 draws"""
    out = np.zeros((len(s), draws), U)
    for k in range(draws):
        s = lcg(s)
        out[:, k] = s
    return out


def surface_records(pos, nrm, prim=None):
    """(n, 24) float32 bdpt_surface records with posW, N and prim set and every other word 0"""
    n = len(pos)
    rec = np.zeros((n, 24), F)
    rec[:, 0:3], rec[:, 4:7] = pos, nrm
    rec.view(np.int32)[:, 23] = 0 if prim is None else prim
    return rec


def ao_oracle(lib, osc, rec, seeds, samples, radius, min_t, alive=None, flags=0):
    """bdpt_ao_query composed from the oracle's hooks on (n, 24) bdpt_surface records.
    -> dict(ao (n,) float32, counts (n,) uint32, seeds_out (n,) uint32, dirs (n, samples, 3) float32, vis (n, samples) bool,
    live (n,) bool); dirs and vis of dead items stay 0 / True."""
    rec = np.ascontiguousarray(rec, F)
    n = len(rec)
    live = rec.view(np.int32)[:, 23] >= 0
    if alive is not None:
        live &= np.asarray(alive) != 0
    s = np.ascontiguousarray(seeds, U).copy()
    counts = np.zeros(n, U)
    dirs, vis = np.zeros((n, samples, 3), F), np.ones((n, samples), bool)
    idx = np.nonzero(live)[0]
    m = len(idx)
    for k in range(samples if m else 0):
        bs_in, bs_out = np.zeros((m, 20), F), np.zeros((m, 16), F)
        bs_in[:, 0:3] = rec[idx, 4:7]
        bs_in.view(U)[:, 17] = s[idx]  # the seed, by value
        lib.oracle_bsdf(bs_in.ctypes.data, m, 1, bs_out.ctypes.data)
        L = bs_out[:, 3:6]
        s[idx] = lcg(lcg(s[idx]))  # getCosHemisphereSample's two draws
        rays = np.zeros((m, 8), F)
        rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = rec[idx, 0:3], L, F(min_t), F(radius)
        prim, tuv = np.zeros(m, np.int32), np.zeros((m, 3), F)
        lib.oracle_trace(osc, rays.ctypes.data, m, 2, flags, prim.ctypes.data, tuv.ctypes.data)
        dirs[idx, k], vis[idx, k] = L, prim < 0
        counts[idx] += (prim < 0).astype(U)
    counts[~live] = samples
    with np.errstate(all="ignore"):
        ao = counts.astype(F) / F(samples)
    return dict(ao=ao, counts=counts, seeds_out=s, dirs=dirs, vis=vis, live=live)


# ---- the float64 reading ---------------------------------------------------------------------------------------------
def _perpendicular(u):
    a = np.abs(u)
    xm = ((a[:, 0] - a[:, 1]) < 0) & ((a[:, 0] - a[:, 2]) < 0)
    ym = ((a[:, 1] - a[:, 2]) < 0) & ~xm
    zm = ~(xm | ym)
    return np.cross(u, np.stack([xm, ym, zm], axis=1).astype(np.float64))


def f64_directions(seeds, nrm, samples):
    """getCosHemisphereSample for `samples` consecutive samples per item in float64 -> (n, samples, 3)"""
    s = np.asarray(seeds, U).copy()
    nrm = np.asarray(nrm, np.float64)
    bitangent = _perpendicular(nrm)
    tangent = np.cross(bitangent, nrm)
    out = np.zeros((len(s), samples, 3))
    for k in range(samples):
        s = lcg(s)
        r0 = (s & U(0x00FFFFFF)).astype(np.float64) / 16777216.0
        s = lcg(s)
        r1 = (s & U(0x00FFFFFF)).astype(np.float64) / 16777216.0
        r, phi = np.sqrt(r0), 2.0 * np.pi * r1
        out[:, k] = (tangent * (r * np.cos(phi))[:, None] + bitangent * (r * np.sin(phi))[:, None] +
                     nrm * np.sqrt(1.0 - r0)[:, None])
    return out


def f64_any_hit(pos, tri, org, dirs, tmin, tmax, chunk=2048):
    """Moeller-Trumbore in float64 over every triangle, the ANY-hit rule: -> (occluded, left_out) per ray.  A ray is left
    out when some candidate lies within F64_TOL of a triangle's edge or of tmin / tmax (no runner-up rule: which triangle
    occludes does not matter)."""
    p = np.asarray(pos, np.float64)
    v0 = p[tri[:, 0]]
    e1, e2 = p[tri[:, 1]] - v0, p[tri[:, 2]] - v0
    occluded, left = np.zeros(len(org), bool), np.zeros(len(org), bool)
    for a in range(0, len(org), chunk):
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
        occluded[a:a + chunk], left[a:a + chunk] = hit.any(axis=1), near.any(axis=1)
    return occluded, left


# ---- numpy-built scenes ----------------------------------------------------------------------------------------------
class QuadScene:
    """Quads (four corners in order, the normal that faces the open side) as a scene description: two triangles each, one
    opaque double-sided material, one point light."""

    def __init__(self, pkg, quads):
        a = pkg.abi
        self.quads = [(np.asarray(c, F), np.asarray(n, F)) for c, n in quads]
        self.pos = np.concatenate([c for c, _ in self.quads]).astype(F)
        self.nrm = np.concatenate([np.tile(n, (4, 1)) for _, n in self.quads]).astype(F)
        nq = len(self.quads)
        base = 4 * np.arange(nq)[:, None]
        self.tri = (base + np.array([[0, 1, 2, 0, 2, 3]])).reshape(-1, 3).astype(np.int64)
        idx = np.ascontiguousarray(self.tri.reshape(-1), U)
        uv = np.zeros((4 * nq, 3), F)
        tri_mat = np.zeros(2 * nq, U)
        mats = (a.Material * 1)()
        for k in range(4):
            mats[0].baseColor[k] = 1.0
        mats[0].alphaThreshold = 0.5
        mats[0].IoR = 1.5
        mats[0].flags = (1 << 3) | (1 << 6) | (1 << 19)  # constant diffuse and specular, double sided, opaque
        mats[0].texBaseColor = mats[0].texSpecular = mats[0].texEmissive = mats[0].texNormal = -1
        lights = (a.Light * 1)()
        lights[0].posW[1] = 0.9
        lights[0].intensity[0] = lights[0].intensity[1] = lights[0].intensity[2] = 1.0
        d = a.SceneDesc()
        d.numVertices, d.numTriangles, d.numMaterials, d.numTextures, d.numLights = 4 * nq, 2 * nq, 1, 0, 1
        fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
        d.positions, d.normals, d.texcoords = fp(self.pos), fp(self.nrm), fp(uv)
        d.indices = idx.ctypes.data_as(C.POINTER(C.c_uint32))
        d.triMaterial = tri_mat.ctypes.data_as(C.POINTER(C.c_uint32))
        d.materials, d.lights = mats, lights
        self.desc, self.keep = d, [idx, uv, tri_mat, mats, lights]
        self.ext = float(np.max(self.pos.max(axis=0) - self.pos.min(axis=0)))

    def surface_points(self, rng, n):
        """n points on the quads, area weighted, a little inside their outlines -> (pos, normal) float32"""
        area = np.array([np.linalg.norm(np.cross(c[1] - c[0], c[3] - c[0])) for c, _ in self.quads])
        q = rng.choice(len(self.quads), size=n, p=area / area.sum())
        st = rng.uniform(0.01, 0.99, size=(n, 2))
        c = np.stack([self.quads[i][0] for i in q]).astype(np.float64)
        p = c[:, 0] + (c[:, 1] - c[:, 0]) * st[:, 0:1] + (c[:, 3] - c[:, 0]) * st[:, 1:2]
        return p.astype(F), np.stack([self.quads[i][1] for i in q]).astype(F)


def _rect(axis, at, lo, hi, normal):
    """the axis-aligned rectangle `axis` = at spanning [lo, hi] in the other two axes"""
    o = [k for k in range(3) if k != axis]
    c = np.zeros((4, 3))
    c[:, axis] = at
    c[:, o[0]] = [lo[0], hi[0], hi[0], lo[0]]
    c[:, o[1]] = [lo[1], lo[1], hi[1], hi[1]]
    n = np.zeros(3)
    n[axis] = normal
    return c, n


def _block(lo, hi):
    """the six faces of an axis-aligned box, normals outward"""
    faces = []
    for axis in range(3):
        o = [k for k in range(3) if k != axis]
        l2, h2 = (lo[o[0]], lo[o[1]]), (hi[o[0]], hi[o[1]])
        faces += [_rect(axis, lo[axis], l2, h2, -1.0), _rect(axis, hi[axis], l2, h2, 1.0)]
    return faces


def room_quads(closed=False, blocks=True):
    """The unit room [-1, 1]^3 seen from +z: floor, ceiling, back and side walls (and the front wall when `closed`), normals
    inward; with `blocks` a short and a tall box standing on the floor (their bottoms coincide with it)."""
    q = [_rect(1, -1.0, (-1, -1), (1, 1), 1.0), _rect(1, 1.0, (-1, -1), (1, 1), -1.0), _rect(2, -1.0, (-1, -1), (1, 1), 1.0),
         _rect(0, -1.0, (-1, -1), (1, 1), 1.0), _rect(0, 1.0, (-1, -1), (1, 1), -1.0)]
    if closed:
        q.append(_rect(2, 1.0, (-1, -1), (1, 1), -1.0))
    if blocks:
        q += _block((0.15, -1.0, 0.05), (0.7, -0.4, 0.6)) + _block((-0.7, -1.0, -0.65), (-0.15, 0.2, -0.1))
    return q


def floor_quads():
    return [_rect(1, 0.0, (-1, -1), (1, 1), 1.0)]
