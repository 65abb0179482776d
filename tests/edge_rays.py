"""Edge-case rays for the traversal tests (tests/test_trace_edge_rays_cpu.py, tests/test_gpu_trace_edge_rays.py): the
scenes, the ray families and a float64 reference.  Plain numpy; the only product code used is the host trace hook
(bdpt_host_bvh_*), whose linear scan (brute = 1) supplies the first-hit distances the interval family is built from and
the answers every tree walk is compared with.

Rays are n x 8 float32 in the oracle / test-hook layout (origin, direction, tmin, tmax).  A batch holds every family of
one scene and as many ordinary random rays as fit, all in one fixed random order, so that in the persistent kernels a
lane with an edge ray retires next to lanes that go on working.  No scene has more than 2000 triangles and no batch more
than MAX_RAYS rays."""
import ctypes as C

import numpy as np

from test_refit_cpu import HostTree, moved_desc

MAX_RAYS = 8192
SCENES = ("soup", "soup64", "grid", "cornell")
MODES = (0, 1, 2)  # closest, closest with back faces culled, any
REFIT_SHIFT = np.array([0.5, 0.0, 0.0], np.float32)
GRID_N = 16        # quads per side
GRID_STEP = 0.125  # vertex spacing: every coordinate is a multiple of 1/8, every midpoint one of 1/16
GRID_OFFSETS = ((0.0, 0.0, 1.0), (0.5, 0.25, 1.0), (-1.0, 2.0, 0.5), (0.0, 1.0, 1.0), (3.0, -3.0, 0.125))  # first: straight down
F64_TOL = 1e-4     # float64 check: margin to a triangle's edge and relative gap to the runner-up below which a ray is left out
F64_MAX_LEFT_OUT = 0.02


class EdgeScene:
    """A scene description with its vertices and triangles as numpy arrays."""

    def __init__(self, name, desc, keep):
        self.name, self.desc, self.keep = name, desc, keep
        self.pos = np.ctypeslib.as_array(desc.positions, shape=(desc.numVertices, 3)).copy()
        self.tri = np.ctypeslib.as_array(desc.indices, shape=(desc.numTriangles, 3)).astype(np.int64)
        assert desc.numTriangles <= 2000
        self.lo, self.hi = self.pos.min(axis=0), self.pos.max(axis=0)
        self.ext = float(np.max(self.hi - self.lo))
        # where ray origins are drawn: the scene box, a flat side of it (the grid's z) opened to half the extent each way
        flat = (self.hi - self.lo) == 0
        self.olo = np.where(flat, self.lo - 0.5 * self.ext, self.lo).astype(np.float32)
        self.ohi = np.where(flat, self.hi + 0.5 * self.ext, self.hi).astype(np.float32)

    def moved(self, pkg, shift):
        p = (self.pos + np.asarray(shift, np.float32)).astype(np.float32)
        return EdgeScene(self.name, moved_desc(pkg, self.desc, p), [self.keep, p])


def grid_desc(pkg):
    """GRID_N x GRID_N quads in z = 0 on multiples of GRID_STEP, quad (i, j) split along the diagonal from its (i, j)
    corner to its (i + 1, j + 1) corner; one opaque material."""
    a = pkg.abi
    m = GRID_N + 1
    j, i = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    pos = np.stack([i.ravel() * GRID_STEP, j.ravel() * GRID_STEP, np.zeros(m * m)], axis=1).astype(np.float32)
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (m * m, 1))
    uv = np.ascontiguousarray(pos / (GRID_N * GRID_STEP), np.float32)
    uv[:, 2] = 0
    qj, qi = np.meshgrid(np.arange(GRID_N), np.arange(GRID_N), indexing="ij")
    v00 = (qj * m + qi).ravel()
    idx = np.stack([v00, v00 + 1, v00 + m + 1, v00, v00 + m + 1, v00 + m], axis=1).astype(np.uint32).reshape(-1)
    tri_mat = np.zeros(2 * GRID_N * GRID_N, np.uint32)
    mats = (a.Material * 1)()
    for k in range(4):
        mats[0].baseColor[k] = 1.0
    mats[0].alphaThreshold = 0.5
    mats[0].IoR = 1.5
    mats[0].flags = (1 << 3) | (1 << 6) | (1 << 19)  # the opaque material of test_bvh_builder._card_scene
    mats[0].texBaseColor = mats[0].texSpecular = mats[0].texEmissive = mats[0].texNormal = -1
    lights = (a.Light * 1)()
    lights[0].posW[2] = 3.0
    lights[0].intensity[0] = lights[0].intensity[1] = lights[0].intensity[2] = 1.0
    d = a.SceneDesc()
    d.numVertices, d.numTriangles, d.numMaterials, d.numTextures, d.numLights = m * m, 2 * GRID_N * GRID_N, 1, 0, 1
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    d.positions, d.normals, d.texcoords = fp(pos), fp(nrm), fp(uv)
    d.indices = idx.ctypes.data_as(C.POINTER(C.c_uint32))
    d.triMaterial = tri_mat.ctypes.data_as(C.POINTER(C.c_uint32))
    d.materials, d.lights = mats, lights
    return d, [pos, nrm, uv, idx, tri_mat, mats, lights]


def make_scene(pkg, name):
    if name in ("soup", "soup64"):
        s = pkg.Scene.soup(3, 2000, 0.2)
        sc = EdgeScene(name, s.desc, [s])
        return sc if name == "soup" else EdgeScene(name, *_moved(pkg, sc, 64.0))
    if name == "grid":
        return EdgeScene(name, *grid_desc(pkg))
    assert name == "cornell"
    s = pkg.Scene.cornell()
    return EdgeScene(name, s.desc, [s])


def _moved(pkg, sc, shift):
    p = (sc.pos + np.float32(shift)).astype(np.float32)
    return moved_desc(pkg, sc.desc, p), [sc.keep, p]


# ---- ray families ---------------------------------------------------------------------------------------------------
def pack(o, d, tmin, tmax):
    n = len(o)
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3], r[:, 3:6] = o, d
    r[:, 6], r[:, 7] = tmin, tmax
    return r


def _origins(sc, rng, n):
    return rng.uniform(sc.olo, sc.ohi, (n, 3)).astype(np.float32)


def _signed_zero_combos():
    """(axis, the direction's three components) for d = +-e_k with every sign of the two zeros: 24 directions"""
    out = []
    for k in range(3):
        for s in (1.0, -1.0):
            for za in (0.0, -0.0):
                for zb in (0.0, -0.0):
                    d = [za, zb]
                    d.insert(k, s)
                    out.append(d)
    return np.array(out, np.float32)


def random_rays(sc, rng, n):
    """The ordinary rays of the other traversal tests: origins in and around the box, normal directions (an eighth of them
    not unit length), half with a short tmax."""
    pad = 0.25 * sc.ext
    o = rng.uniform(sc.olo - pad, sc.ohi + pad, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[: n // 8] *= rng.uniform(0.1, 5.0, (n // 8, 1)).astype(np.float32)
    tmax = np.full(n, 1e38, np.float32)
    tmax[n // 2:] = rng.uniform(0.05, 1.0, n - n // 2).astype(np.float32) * sc.ext
    return pack(o, d, 1e-4 * sc.ext, tmax)


def axis_rays(sc, rng, per):
    dirs = np.repeat(_signed_zero_combos(), per, axis=0)
    return pack(_origins(sc, rng, len(dirs)), dirs, 1e-4 * sc.ext, 1e38)


def axis_rays_on_vertices(sc, rng, per):
    """The grid: origins whose x and y are vertex coordinates (so they lie on planes of the tree's boxes while the
    direction's component along that axis is a signed zero), z in {-1, -0.5, 0, 0.5, 1}."""
    dirs = np.repeat(_signed_zero_combos(), per, axis=0)
    n = len(dirs)
    o = sc.pos[rng.integers(0, len(sc.pos), n)].copy()
    o[:, 2] = rng.choice(np.array([-1.0, -0.5, 0.0, 0.5, 1.0], np.float32), n)
    return pack(o, dirs, 1e-4 * sc.ext, 1e38)


def partly_zero_rays(sc, rng, per):
    """One or two components of a random direction replaced by +0.0 / -0.0: 6 + 12 patterns."""
    pats = []
    for k in range(3):
        for z in (0.0, -0.0):
            pats.append({k: z})
    for k in range(3):
        a, b = [x for x in range(3) if x != k]
        for za in (0.0, -0.0):
            for zb in (0.0, -0.0):
                pats.append({a: za, b: zb})
    d = rng.normal(size=(len(pats) * per, 3)).astype(np.float32)
    for i, p in enumerate(pats):
        for k, z in p.items():
            d[i * per:(i + 1) * per, k] = z
    return pack(_origins(sc, rng, len(d)), d, 1e-4 * sc.ext, 1e38)


def wall_normal_rays(sc, rng, per):
    """From points on every triangle along -N and +N, N the fp32 geometric normal; the direction is written as the
    negation of a vector, so that a zero component of an axis-aligned wall's normal arrives with either sign."""
    a, b, c = (sc.pos[sc.tri[:, k]] for k in range(3))
    n = np.cross(b - a, c - a).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True).astype(np.float32)
    t = np.repeat(np.arange(len(sc.tri)), per)
    w = rng.uniform(0.1, 1.0, (len(t), 3))
    w /= w.sum(axis=1, keepdims=True)
    p = (w[:, 0:1] * a[t] + w[:, 1:2] * b[t] + w[:, 2:3] * c[t]).astype(np.float32)
    minus = np.negative(n[t])
    return pack(np.concatenate([p, p]), np.concatenate([minus, np.negative(minus)]), 1e-4 * sc.ext, 1e38)


def aimed_rays(sc, rng, n, what):
    """d = target - o in fp32, the target a vertex or the fp32 midpoint of a triangle's edge"""
    if what == "vertex":
        target = sc.pos[rng.integers(0, len(sc.pos), n)]
    else:
        t, e = rng.integers(0, len(sc.tri), n), rng.integers(0, 3, n)
        target = (np.float32(0.5) * (sc.pos[sc.tri[t, e]] + sc.pos[sc.tri[t, (e + 1) % 3]])).astype(np.float32)
    o = _origins(sc, rng, n)
    return pack(o, (target - o).astype(np.float32), 1e-4 * sc.ext, 1e38)


def grid_targets(sc):
    """Every vertex, every edge midpoint and every quad-diagonal midpoint of the grid: together the whole 1/16 lattice
    over it (289 + 544 + 256 = 33 x 33 points), from the grid's corner (itself dyadic, also after the refit's shift)."""
    m = 2 * GRID_N + 1
    y, x = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    lattice = np.stack([x.ravel() * (GRID_STEP / 2), y.ravel() * (GRID_STEP / 2), np.zeros(m * m)], axis=1).astype(np.float32)
    return sc.lo + lattice


def grid_dyadic_rays(sc):
    """o = target + offset, d = -offset: every quantity in Moeller-Trumbore is a dyadic rational of a few bits, so
    fp32 evaluates it exactly: t = 1, and the hit is shared by every triangle that contains the target."""
    tg = grid_targets(sc)
    out = []
    for off in GRID_OFFSETS:
        off = np.array(off, np.float32)
        out.append(pack(tg + off, np.tile(np.negative(off), (len(tg), 1)), 1e-4, 1e38))
    return np.concatenate(out)


def interval_rays(sc, rng, n, scan):
    """Four copies of n rays that hit: tmax equal to the first hit's t bit for bit (a miss: t < tmax is strict), tmin
    equal to it (the first hit is skipped), tmax = inf, and a negative tmin."""
    cand = random_rays(sc, rng, 4 * n)
    cand[:, 7] = 1e38
    prim, tuv = scan(cand)
    base = cand[prim >= 0][:n]
    t = tuv[prim >= 0][:n, 0]
    assert len(base) >= n // 4, "the interval family needs rays that hit"
    a, b, c, d = base.copy(), base.copy(), base.copy(), base.copy()
    a[:, 7] = t
    b[:, 6] = t
    c[:, 7] = np.inf
    d[:, 6] = -0.5 * sc.ext
    return np.concatenate([a, b, c, d])


def scaled_rays(sc, rng, n):
    """Direction lengths 1e-20, 1e20 and 1e30 (tmin = 0: with the long directions every hit has a tiny t)"""
    out = []
    for s in (1e-20, 1e20, 1e30):
        r = random_rays(sc, rng, n)
        r[:, 3:6] *= np.float32(s)
        r[:, 6], r[:, 7] = 0.0, 1e38
        out.append(r)
    return np.concatenate(out)


def invalid_rays(sc, rng):
    r = random_rays(sc, rng, 4)
    r[:, 7] = 1e38
    r[0, 3:6] = 0.0     # zero direction
    r[1, 3:6] = np.nan  # NaN direction
    r[2, 7] = 0.0       # tmax <= tmin
    r[3, 0] = np.nan    # NaN origin
    return r


class Batch:
    def __init__(self, rays, family, names):
        self.rays, self.family, self.names = rays, family, names

    def of(self, name):
        return self.family == self.names.index(name)

    def tally(self, bad):
        """mismatches per family, for an assertion's message"""
        return {n: int(bad[self.family == i].sum()) for i, n in enumerate(self.names) if bad[self.family == i].any()}


def families(sc, scan, seed=1):
    rng = np.random.default_rng(seed)
    small = sc.name == "grid"  # the grid's dyadic family alone has 5445 rays
    per = 16 if small else 32
    fam = {"axis": axis_rays(sc, rng, per), "partly_zero": partly_zero_rays(sc, rng, per)}
    if sc.name == "grid":
        fam["axis_on_vertices"] = axis_rays_on_vertices(sc, rng, per)
        fam["dyadic"] = grid_dyadic_rays(sc)
    elif sc.name == "cornell":
        fam["walls"] = wall_normal_rays(sc, rng, 16)
    if sc.name != "grid":
        fam["at_vertices"] = aimed_rays(sc, rng, 512, "vertex")
        fam["at_edge_midpoints"] = aimed_rays(sc, rng, 512, "edge")
    fam["interval"] = interval_rays(sc, rng, 64 if small else 256, scan)
    fam["scaled"] = scaled_rays(sc, rng, 64 if small else 192)
    fam["invalid"] = invalid_rays(sc, rng)
    return fam


def mixed_batch(sc, scan, seed=1):
    fam = families(sc, scan, seed)
    n_edge = sum(len(r) for r in fam.values())
    assert n_edge < MAX_RAYS
    rng = np.random.default_rng(seed + 1000)
    fam["random"] = random_rays(sc, rng, min(n_edge, MAX_RAYS - n_edge))
    names = list(fam)
    rays = np.concatenate([fam[k] for k in names])
    label = np.concatenate([np.full(len(fam[k]), i, np.int32) for i, k in enumerate(names)])
    order = rng.permutation(len(rays))
    return Batch(np.ascontiguousarray(rays[order]), label[order], names)


# ---- float64 reference ----------------------------------------------------------------------------------------------
def reference_f64(sc, rays, chunk=256):
    """Moeller-Trumbore in float64 over every triangle.  Returns (prim, left_out): the closest hit's primitive (-1: none)
    and the rays whose answer fp32 may legitimately give differently: some candidate (a triangle the ray meets within
    F64_TOL of its outline and of the interval) lies within F64_TOL of one of its edges or of tmin / tmax, or the
    runner-up is within F64_TOL relative in t."""
    p = sc.pos.astype(np.float64)
    v0 = p[sc.tri[:, 0]]
    e1, e2 = p[sc.tri[:, 1]] - v0, p[sc.tri[:, 2]] - v0
    prim = np.full(len(rays), -1, np.int64)
    left = np.zeros(len(rays), bool)
    for s in range(0, len(rays), chunk):
        r = rays[s:s + chunk].astype(np.float64)
        o, d, tmin, tmax = r[:, None, 0:3], r[:, None, 3:6], r[:, 6:7], r[:, 7:8]
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
            cand = ok & (margin > -F64_TOL) & (t > tmin - F64_TOL * np.abs(tmin)) & (t < tmax + F64_TOL * np.abs(tmax))
            near = cand & ((np.abs(margin) < F64_TOL) | (np.abs(t - tmin) <= F64_TOL * np.abs(t)) | (np.abs(t - tmax) <= F64_TOL * np.abs(t)))
        th = np.where(hit, t, np.inf)
        first = th.argmin(axis=1)
        t1 = th[np.arange(len(r)), first]
        any_hit = np.isfinite(t1)
        th[np.arange(len(r)), first] = np.inf
        t2 = th.min(axis=1)
        gap = np.where(np.isfinite(t2), t2, 0.0) - np.where(any_hit, t1, 0.0)
        close = any_hit & np.isfinite(t2) & (gap <= F64_TOL * np.abs(t1))
        prim[s:s + chunk] = np.where(any_hit, first, -1)
        left[s:s + chunk] = near.any(axis=1) | close
    return prim, left


# ---- cases: one scene, its batch and the linear scan's answers, made once and shared ---------------------------------
class Case:
    def __init__(self, pkg, name, moved):
        sc = make_scene(pkg, name)
        self.sc = sc.moved(pkg, REFIT_SHIFT) if moved else sc
        self.built = sc  # the scene the trees are built from (the refit tests move them to self.sc)
        tree = HostTree(pkg, self.sc.desc, 0.0, 0.0, 0)
        self.batch = mixed_batch(self.sc, lambda r: tree.trace(r, 0, 1))
        self.scan = {m: tree.trace(self.batch.rays, m, 1) for m in MODES}
        tree.close()


_cases = {}


def case(pkg, name, moved=False):
    if (name, moved) not in _cases:
        _cases[(name, moved)] = Case(pkg, name, moved)
    return _cases[(name, moved)]


def differs_from_scan(c, mode, prim, tuv):
    """per ray: the answer is not the linear scan's (closest: prim and the bits of t / u / v; any: hit or miss)"""
    sp, st = c.scan[mode]
    if mode == 2:
        return (prim >= 0) != (sp >= 0)
    return (prim != sp) | (np.ascontiguousarray(tuv, np.float32).view(np.uint32) != st.view(np.uint32)).any(axis=1)


def assert_like_scan(c, mode, prim, tuv, what):
    bad = differs_from_scan(c, mode, prim, tuv)
    if bad.any():
        hits = {n: (int((c.scan[mode][0][c.batch.of(n)] >= 0).sum()), int((prim[c.batch.of(n)] >= 0).sum())) for n in c.batch.tally(bad)}
        raise AssertionError(f"{c.sc.name} {what} mode {mode}: rays that differ from the scan per family {c.batch.tally(bad)}; "
                             f"(scan hits, hits here) {hits}")
