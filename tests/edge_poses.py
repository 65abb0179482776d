"""Edge-case poses for the animated path (tests/test_edge_poses_cpu.py, tests/test_gpu_edge_poses.py): deterministic
fp32 positions that a bone, a morph or a world offset can reach — far from the origin, huge, tiny, flattened onto a plane,
collapsed to a line or a point, mirrored, permuted, with -0.0 coordinates, with some triangles collapsed — and the ray
families that go with each pose.  Plain numpy; the only product code used is the host hooks (bdpt_host_bvh_*), whose linear
scan (brute = 1) defines the right answer.

The two scenes are the smallest here known to have split, clipped and dropped references (asserted by `tree`).  Every pose
carries a predicate that proves it reaches its edge (`Pose.reaches`), and a class that says what the scan itself can still
see there:
  "hits"   the scan hits the posed scene; the tree must answer as the scan does, and the test asserts a hit count
  "blind"  the scan hits nothing (the fp32 ray / triangle test overflows, underflows or has nothing of positive area left);
           the tree must hit nothing either
  "refused" outside the range bdpt.h "Animated scenes" states for positions: the host paths answer BDPT_E_INVALID

Rays are n x 8 float32 in the test-hook layout (origin, direction, tmin, tmax); `to_device_rays` reorders them into the
bdpt_ray layout (origin, tmin, direction, tmax)."""
import numpy as np

import edge_rays as er
from test_refit_cpu import HostTree, moved_desc, positions_of

SCENES = ("atrium_split", "courtyard_clipped")
KINDS = ("plain", "pieces")
MODES = (0, 1, 2)
RAYS_PER_MODE = 20480  # at least 20 k per mode and pose


def fixture(pkg, which):
    """(scene, host budgets) — test_refit_pieces_cpu.fixture_with_pieces"""
    if which == "atrium_split":
        return pkg.Scene.atrium(2, 6000), (1.0, 4.0, 1)
    return pkg.Scene.courtyard(2, 6000, 0.6), (-1.0, -1.0, 1)


def tree(pkg, which, scene, budgets, kind, cls=HostTree):
    """A host tree of the scene as built, with the piece regions for kind == "pieces"; asserts that it has pieces."""
    t = cls(pkg, scene.desc, *budgets)
    if which == "atrium_split":
        assert t.info.numReferences > scene.desc.numTriangles
    else:
        assert t.info.numReferences != scene.desc.numTriangles or t.info.numDropped > 0
    if kind == "pieces":
        assert t.lib.bdpt_host_bvh_refit_pieces(t.h) == 0
    return t


# ---- poses ----------------------------------------------------------------------------------------------------------
class Pose:
    def __init__(self, name, pos, cls, reaches, flat=None):
        self.name, self.pos, self.cls, self.reaches = name, np.ascontiguousarray(pos, np.float32), cls, reaches
        self.flat = flat  # None, ("plane", point, unit normal) or ("line", point, unit direction), float64


def _box(p):
    return p.min(axis=0).astype(np.float64), p.max(axis=0).astype(np.float64)


def _dot(x, a):
    """rows of x times the vector a, in one fixed order of operations (a BLAS product may round otherwise elsewhere)"""
    return x[:, 0] * a[0] + x[:, 1] * a[1] + x[:, 2] * a[2]


def _ext(p):
    lo, hi = _box(p)
    return float(np.max(hi - lo))


FAR = {"far_1e3": 1e3, "far_3e4": 3e4, "far_1e5": 1e5, "far_1e7": 1e7}
SCALE = {"scale_1e6": 1e6, "scale_1e10": 1e10, "scale_1e13": 1e13, "scale_1e15": 1e15, "scale_1e19": 1e19, "scale_1e-20": 1e-20,
         "scale_1e-36": 1e-36}
FAR_DIR = np.array([1.0, 0.5, -0.25])  # every axis far away, each with another ulp
OBLIQUE = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
NAMES = (("built",) + tuple(FAR) + tuple(SCALE) + ("flat_centre", "flat_zero", "flat_oblique", "line", "point", "mirror_x", "permuted",
                                                   "neg_zero", "some_collapsed"))
# what the scan itself still sees (module docstring); everything not named here is "hits"
BLIND = ("far_1e7", "scale_1e15", "scale_1e-20", "scale_1e-36", "line", "point")
REFUSED = ("scale_1e19",)


def tri_classes(pos, tri):
    """float64 classes of the posed triangles: (two corners equal, collinear but distinct, relative height h / longest edge)"""
    p = pos.astype(np.float64)
    a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    two = (a == b).all(1) | (b == c).all(1) | (a == c).all(1)
    with np.errstate(all="ignore"):
        s = max(float(np.abs(p).max()), 1e-300)
        a, b, c = a / s, b / s, c / s
        longest = np.sqrt(np.maximum(np.maximum(((b - a) ** 2).sum(1), ((c - a) ** 2).sum(1)), ((c - b) ** 2).sum(1)))
        area2 = np.sqrt((np.cross(b - a, c - a) ** 2).sum(1))
        h = np.where(longest > 0, area2 / np.maximum(longest, 1e-300) ** 2, 0.0)
    return two, (~two) & (h == 0), h


def _some_collapsed(p0, tri, seed=5):
    """10 % of the triangles with two equal corners, 10 % with the third corner on the line of the other two, 10 % slivers
    of relative height 1e-7, the rest as built (but for the corners they share with those).  One corner of a taken triangle
    moves; no corner of a taken triangle moves afterwards."""
    rng = np.random.default_rng(seed)
    p = p0.astype(np.float64)
    taken = np.zeros(len(p0), bool)  # corners of the triangles taken so far: they stay where they are
    want = len(tri) // 10
    picked = {0: [], 1: [], 2: []}
    kind = 0
    for t in rng.permutation(len(tri)):
        if kind == 3:
            break
        i, j, k = tri[t]
        e = p[j] - p[i]
        if len({i, j, k}) < 3 or taken[j if kind == 0 else k] or not e.any():
            continue
        if kind == 0:
            p[j] = p[i]
        elif kind == 1:
            p[k] = p[i] + 0.5 * e  # (the midpoint of two fp32 points: collinear up to fp32 rounding, often exactly)
        else:
            side = np.cross(np.cross(e, p[k] - p[i]), e)
            if not side.any():
                continue
            p[k] = p[i] + 0.5 * e + 1e-7 * np.linalg.norm(e) * side / np.linalg.norm(side)
        taken[[i, j, k]] = True
        picked[kind].append(t)
        if len(picked[kind]) == want:
            kind += 1
    assert kind == 3, "the scene has too few independent triangles"
    return p.astype(np.float32), {k: np.array(v) for k, v in picked.items()}


def make_pose(name, p0, tri):
    """The pose `name` of the scene (p0: fp32 positions as built, tri: its triangles)."""
    lo, hi = _box(p0)
    ctr, ext = 0.5 * (lo + hi), float(np.max(hi - lo))
    p = p0.astype(np.float64)
    cls = "refused" if name in REFUSED else ("blind" if name in BLIND else "hits")
    if name == "built":
        return Pose(name, p0, cls, lambda q: np.array_equal(q, p0))
    if name in FAR:
        k = FAR[name]
        # ulp of the largest coordinate against the extent: 1e3 -> 6e-5, 1e5 -> 8e-3, 1e7 -> about one
        return Pose(name, p + k * ext * FAR_DIR, cls,
                    lambda q: float(np.spacing(np.float32(np.abs(q).max()))) >= 0.5 * k * 2.0 ** -24 * ext and np.isfinite(q).all())
    if name in SCALE:
        s = SCALE[name]
        q = (p * s).astype(np.float32)
        if s == 1e19:
            ok = lambda q: np.isfinite(q).all() and _ext(q) ** 2 > float(np.finfo(np.float32).max)  # dx * dx overflows in fp32
        elif s == 1e-36:
            ok = lambda q: (np.abs(q[q != 0]) < np.finfo(np.float32).tiny).any()  # subnormal coordinates
        else:
            ok = lambda q: np.isfinite(q).all() and _ext(q) > 0
        return Pose(name, q, cls, ok)
    if name in ("flat_centre", "flat_zero"):
        q = p.copy()
        q[:, 2] = ctr[2] if name == "flat_centre" else 0.0
        z = float(np.float32(q[0, 2]))
        return Pose(name, q, cls, lambda q: (q[:, 2] == q[0, 2]).all(), ("plane", np.array([ctr[0], ctr[1], z]), np.array([0.0, 0.0, 1.0])))
    if name == "flat_oblique":
        q = p - _dot(p - ctr, OBLIQUE)[:, None] * OBLIQUE
        return Pose(name, q, cls, lambda q: np.abs(_dot(q.astype(np.float64) - ctr, OBLIQUE)).max() <= 4 * np.spacing(np.float32(np.abs(q).max())),
                    ("plane", ctr, OBLIQUE))
    if name == "line":  # (along x: every triangle exactly collinear in fp32 — on an oblique line they are slivers of fp32 rounding)
        q = p.copy()
        q[:, 1:3] = ctr[1:3]
        at = np.array([ctr[0], float(np.float32(ctr[1])), float(np.float32(ctr[2]))])
        return Pose(name, q, cls, lambda q: tri_classes(q, tri)[2].max() == 0 and _ext(q) > 0, ("line", at, np.array([1.0, 0.0, 0.0])))
    if name == "point":
        return Pose(name, np.tile(ctr, (len(p0), 1)), cls, lambda q: (q == q[0]).all())
    if name == "mirror_x":
        q = p.copy()
        q[:, 0] = lo[0] + hi[0] - q[:, 0]
        return Pose(name, q, cls, lambda q: np.allclose(q[:, 0].astype(np.float64) + p[:, 0], lo[0] + hi[0], atol=1e-6 * ext))
    if name == "permuted":
        perm = np.random.default_rng(4).permutation(len(p0))
        return Pose(name, p0[perm], cls, lambda q: np.linalg.norm(q.astype(np.float64) - p, axis=1).mean() > 0.2 * ext)
    if name == "neg_zero":
        q = p0.copy()
        q[np.abs(q) < 0.02 * ext] = np.float32(-0.0)
        return Pose(name, q, cls, lambda q: int(((q == 0) & np.signbit(q)).sum()) >= 100)
    assert name == "some_collapsed"
    q, picked = _some_collapsed(p0, tri)

    def ok(q):
        two, col, h = tri_classes(q, tri)
        # (a height of 1e-7 of an edge lies below the fp32 spacing of most corners: rounded to fp32 a sliver keeps a height
        # of up to that spacing, 1e-5 of its longest edge at the most, and some come out exactly collinear)
        return (two[picked[0]].all() and (h[picked[1]] < 1e-5).all() and (h[picked[2]] < 1e-5).all() and (h[picked[2]] > 0).any()
                and min(len(v) for v in picked.values()) == len(tri) // 10)
    return Pose(name, q, cls, ok)


# ---- documented limits (include/bdpt.h "Animated scenes") ----------------------------------------------------------------
# Directions with a zero component: the slab test multiplies a node's scale (a power of two, extent / 254 rounded up) by
# the clamped reciprocal 1e30, which overflows from 2^29 on, i.e. for a node wider than 254 * 2^28 = 6.8e10.  The contract
# is stated for scenes no wider than 2^35 (3.4e10); wider poses get no signed-zero families.
ZERO_DIR_MAX_EXTENT = 2.0 ** 35
# Ill-conditioned hits: Moeller-Trumbore's (u, v) carry an error of some 4 eps / c of an edge, c = |e1 . (d x e2)| /
# (|e1| |e2| |d|) the sine of the triangle's corner times the cosine between ray and normal.  The boxes are padded by 2e-5
# of the diagonal, so from c < 4 * 2^-24 / 2e-5 = 1.2e-2 on the point the scan reports can lie outside the box of the
# triangle it reports: a needle (edges parallel up to rounding; its determinant is noise), a sliver, or a ray inside a
# triangle's plane.  Below 2^-6 the scan's answer is not binding, and a ray that differs is excused when the SCAN's
# triangle is that ill-conditioned for it, in float64.
ILL_CONDITIONED = 2.0 ** -6


def _edges64(pos, tri, prims):
    a, b, c = (pos[tri[prims, k]] for k in range(3))
    with np.errstate(all="ignore"):
        return a.astype(np.float64), (b - a).astype(np.float64), (c - a).astype(np.float64)  # (the record's fp32 edges)


def conditioning(pos, tri, rays, prims):
    """c of the pairs (ray i, triangle prims[i]) in float64; inf where prims[i] < 0"""
    ok = prims >= 0
    _, e1, e2 = _edges64(pos, tri, np.where(ok, prims, 0))
    d = rays[:, 3:6].astype(np.float64)
    with np.errstate(all="ignore"):
        c = np.abs((e1 * np.cross(d, e2)).sum(1)) / (np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1) * np.linalg.norm(d, axis=1))
    return np.where(ok & np.isfinite(c), c, np.where(ok, 0.0, np.inf))


def any_ill_conditioned_candidate(pos, tri, ray):
    """any-hit answers name no triangle: is there a triangle that is ill-conditioned for the ray and that float64 meets
    inside the ray's interval within a quarter of its edges?"""
    v0, e1, e2 = _edges64(pos, tri, np.arange(len(tri)))
    o, d, tmin, tmax = ray[0:3].astype(np.float64), ray[3:6].astype(np.float64), float(ray[6]), float(ray[7])
    with np.errstate(all="ignore"):
        pv = np.cross(d, e2)
        det = (e1 * pv).sum(1)
        c = np.abs(det) / (np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1) * np.linalg.norm(d))
        tv = o - v0
        u = (tv * pv).sum(1) / det
        qv = np.cross(tv, e1)
        v = _dot(qv, d) / det
        t = (e2 * qv).sum(1) / det
        near = (u > -0.25) & (v > -0.25) & (u + v < 1.5) & (t > tmin - 1e-3 * abs(tmin)) & (t < tmax * (1 + 1e-3))
    return bool(((c < ILL_CONDITIONED) & (near | ~np.isfinite(t))).any())


# ---- rays -----------------------------------------------------------------------------------------------------------
class _RayScene:
    """what the ray families of edge_rays.py ask of a scene: where origins are drawn and the extent"""

    def __init__(self, pos):
        lo, hi = _box(pos)
        ext = float(np.max(hi - lo))
        if not ext > 0:  # a point: rays from one ulp-sized neighbourhood scale up
            ext = max(float(np.abs(pos).max()), 1.0)
        self.ext = ext
        flat = (hi - lo) < 1e-3 * ext
        self.olo = np.where(flat, lo - 0.5 * ext, lo)
        self.ohi = np.where(flat, hi + 0.5 * ext, hi)


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _bary_points(rng, pos, tri, n):
    t = rng.integers(0, len(tri), n)
    w = rng.uniform(0.05, 1.0, (n, 3))
    w /= w.sum(axis=1, keepdims=True)
    p = pos.astype(np.float64)
    with np.errstate(all="ignore"):
        return w[:, 0:1] * p[tri[t, 0]] + w[:, 1:2] * p[tri[t, 1]] + w[:, 2:3] * p[tri[t, 2]]


def _f32(x):
    with np.errstate(all="ignore"):
        return np.asarray(x, np.float64).astype(np.float32)


def rays_for(pose, tri, seed=7):
    """(rays, family labels, family names) for one pose: RAYS_PER_MODE rays, the same for every mode (mode 2 gets a
    finite tmax on half of the uniform family through the rays themselves)."""
    rng = np.random.default_rng(seed)
    rs = _RayScene(pose.pos)
    tmin = 1e-4 * rs.ext
    fam = {}
    if rs.ext <= ZERO_DIR_MAX_EXTENT:
        fam["axis"] = er.axis_rays(rs, rng, 32)
        fam["partly_zero"] = er.partly_zero_rays(rs, rng, 32)
    n = 4096
    target = _bary_points(rng, pose.pos, tri, n)
    o = rng.uniform(rs.olo, rs.ohi, (n, 3))
    d = target - _f32(o).astype(np.float64)
    with np.errstate(all="ignore"):
        d = np.where(np.isfinite(d / np.linalg.norm(d, axis=1, keepdims=True)), d / np.linalg.norm(d, axis=1, keepdims=True), OBLIQUE)
    fam["aimed"] = er.pack(_f32(o), _f32(d), tmin, 1e38)  # (unit length, so that tmin means the same at every scale)
    fam["on_geometry"] = er.pack(_f32(_bary_points(rng, pose.pos, tri, n)), _f32(_unit(rng, n)), tmin, 1e38)
    if pose.flat is not None:
        n = 2048
        what, at, ax = pose.flat
        o = rng.uniform(rs.olo, rs.ohi, (n, 3))
        if what == "plane":  # origins and directions inside the plane
            o = o - _dot(o - at, ax)[:, None] * ax
            d = _unit(rng, n)
            d = d - _dot(d, ax)[:, None] * ax
        else:  # along the line, from points on it
            o = at + _dot(o - at, ax)[:, None] * ax
            d = np.where(rng.uniform(size=(n, 1)) < 0.5, 1.0, -1.0) * ax
        fam["inside"] = er.pack(_f32(o), _f32(d), tmin, 1e38)
    n = RAYS_PER_MODE - sum(len(r) for r in fam.values())
    pad = 0.25 * rs.ext
    u = er.pack(_f32(rng.uniform(rs.olo - pad, rs.ohi + pad, (n, 3))), _f32(_unit(rng, n)), tmin, 1e38)
    u[n // 2:, 7] = _f32(rng.uniform(0.05, 1.0, n - n // 2) * rs.ext)
    fam["uniform"] = u
    names = list(fam)
    rays = np.concatenate([fam[k] for k in names])
    label = np.concatenate([np.full(len(fam[k]), i, np.int32) for i, k in enumerate(names)])
    order = rng.permutation(len(rays))
    assert len(rays) == RAYS_PER_MODE
    return np.ascontiguousarray(rays[order]), label[order], names


def to_device_rays(rays):
    r = np.empty_like(rays)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = rays[:, 0:3], rays[:, 6], rays[:, 3:6], rays[:, 7]
    return r


# ---- cases: one scene at one pose, its rays and the scan's answers, made once and shared ----------------------------
class Case:
    def __init__(self, pkg, which, name, n=RAYS_PER_MODE):
        self.which, self.name = which, name
        self.scene, self.budgets = fixture(pkg, which)
        self.p0 = positions_of(self.scene.desc)
        self.tri = np.ctypeslib.as_array(self.scene.desc.indices, shape=(self.scene.desc.numTriangles, 3)).astype(np.int64)
        self.pose = make_pose(name, self.p0, self.tri)
        assert self.pose.reaches(self.pose.pos), f"{which} {name}: the pose does not reach its edge"
        self.rays, self.family, self.names = rays_for(self.pose, self.tri)
        self.rays, self.family = self.rays[:n], self.family[:n]  # (in one fixed random order: a prefix holds every family)
        self.desc = moved_desc(pkg, self.scene.desc, self.pose.pos)  # the scene at the pose (for a fresh build)
        self.scan = None
        if self.pose.cls != "refused":
            t = HostTree(pkg, self.scene.desc, 0.0, 0.0, 0)  # (the scan reads the positions, not the tree)
            t.refit(self.pose.pos)
            self.scan = {m: t.trace(self.rays, m, 1) for m in MODES}
            t.close()

    def differs(self, mode, prim, tuv):
        sp, st = self.scan[mode]
        if mode == 2:
            return (prim >= 0) != (sp >= 0)
        return (prim != sp) | (np.ascontiguousarray(tuv, np.float32).view(np.uint32) != st.view(np.uint32)).any(axis=1)

    def excused(self, mode, bad):
        """of the rays in `bad`, those the documented limit ILL_CONDITIONED excuses"""
        out = np.zeros(len(bad), bool)
        if not bad.any():
            return out
        if mode == 2:
            for i in np.flatnonzero(bad):
                out[i] = any_ill_conditioned_candidate(self.pose.pos, self.tri, self.rays[i])
            return out
        return bad & (conditioning(self.pose.pos, self.tri, self.rays, self.scan[mode][0].astype(np.int64)) < ILL_CONDITIONED)

    def tally(self, bad):
        return {n: int(bad[self.family == i].sum()) for i, n in enumerate(self.names) if bad[self.family == i].any()}


_cases = {}


def case(pkg, which, name, n=RAYS_PER_MODE):
    """n: the first n rays of the pose's batch only (the GPU tests, which take seconds)"""
    if (which, name, n) not in _cases:
        _cases[(which, name, n)] = Case(pkg, which, name, n)
    return _cases[(which, name, n)]


# ---- skin rigs that reach such poses on the device (bdpt_set_skin / bdpt_update_skinned, bdpt_host_skin) -------------
def _bone(scale=(1.0, 1.0, 1.0), about=(0.0, 0.0, 0.0), shift=(0.0, 0.0, 0.0)):
    """row-vector bone (pos' = (pos, 1) . M, m[4 r + c]): scale about a point, then a translation; float64, rounded once"""
    m = np.zeros((4, 4))
    s, a = np.asarray(scale, np.float64), np.asarray(about, np.float64)
    m[0, 0], m[1, 1], m[2, 2], m[3, 3] = s[0], s[1], s[2], 1.0
    m[3, 0:3] = a - a * s + np.asarray(shift, np.float64)
    return m.reshape(16)


class SkinRig:
    def __init__(self, name, W, I, bones, kind, reaches):
        self.name, self.kind, self.reaches = name, kind, reaches  # kind: "bits" or "class" (zero / inf / NaN / sign only)
        self.W, self.I = np.ascontiguousarray(W, np.float32), np.ascontiguousarray(I, np.uint16)
        self.bones = np.ascontiguousarray(np.asarray(bones).reshape(-1, 16), np.float32)
        self.num_bones = len(self.bones)


def skin_rigs(p0):
    """Rigs without normals (no inverse transpose needed).  Every vertex hangs on the LAST bone of its palette with
    weight one unless the rig says otherwise; the other bones of a palette are the identity."""
    nv = len(p0)
    lo, hi = _box(p0)
    ctr, ext = 0.5 * (lo + hi), float(np.max(hi - lo))
    one = np.zeros((nv, 4), np.float32)
    one[:, 0] = 1.0

    def on_last(nb):
        ids = np.zeros((nv, 4), np.uint16)
        ids[:, 0] = nb - 1
        return ids

    def palette(nb, last):
        return np.stack([_bone()] * (nb - 1) + [last])

    rigs = []
    flat = lambda axes: (lambda q: all((q[:, a] == q[0, a]).all() for a in axes) and np.isfinite(q).all())
    for name, scale, axes in (("zero_z", (1, 1, 0), (2,)), ("zero_yz", (1, 0, 0), (1, 2)), ("zero_xyz", (0, 0, 0), (0, 1, 2))):
        rigs.append(SkinRig(name, one, on_last(2), palette(2, _bone(scale, ctr)), "bits", flat(axes)))
    rigs.append(SkinRig("mirror_x", one, on_last(3), palette(3, _bone((-1, 1, 1), ctr)), "bits",
                        lambda q: np.allclose(q[:, 0].astype(np.float64) + p0[:, 0], 2 * ctr[0], atol=1e-5 * ext)))
    rigs.append(SkinRig("far_1e5", one, on_last(2), palette(2, _bone(shift=1e5 * ext * FAR_DIR)), "bits",
                        lambda q: np.abs(q).min() > 1e4 * ext and np.isfinite(q).all()))
    w = one.copy()
    w[:, 0], w[:, 1] = 0.75, -0.75
    ids = on_last(2)
    ids[:, 1] = 1  # the same bone with w and -w: the blend cancels exactly
    rigs.append(SkinRig("cancelling", w, ids, palette(2, _bone((2, 2, 2), ctr)), "class", lambda q: (q == 0).all()))
    w = one.copy()
    w[:, 0] = 1e-40
    rigs.append(SkinRig("subnormal_weights", w, on_last(1), palette(1, _bone()), "bits", lambda q: (np.abs(q) < 1e-37).all()))
    w = one.copy()
    w[:, 0], w[:, 1] = 3e38, 3e38
    ids = on_last(2)
    rigs.append(SkinRig("overflowing", w, ids, palette(2, _bone()), "class", lambda q: not np.isfinite(q).any()))
    for nb in (1, 64, 65):  # around the palette size the kernel stages in LDS
        rigs.append(SkinRig(f"palette_{nb}_zero_z", one, on_last(nb), palette(nb, _bone((1, 1, 0), ctr)), "bits", flat((2,))))
    return rigs


def value_class(a):
    """0 zero, 1 finite, 2 inf, 3 NaN — plus 4 for a set sign bit of anything but a NaN"""
    a = np.ascontiguousarray(a, np.float32)
    c = np.where(np.isnan(a), 3, np.where(np.isinf(a), 2, np.where(a == 0, 0, 1)))
    return c + np.where(np.isnan(a), 0, 4 * np.signbit(a))


# ---- morph rigs (bdpt_set_morph / bdpt_update_morphed, bdpt_host_morph) ----------------------------------------------
MORPH_ENTRIES = (1, 3, 4, 5, 8, 9)  # entries per vertex: around the deform pass's batch of four


class MorphRig:
    def __init__(self, name, tg, weights, base, kind, reaches, skin=None):
        self.name, self.tg, self.kind, self.reaches, self.skin = name, tg, kind, reaches, skin
        self.weights = np.ascontiguousarray(weights, np.float32)
        self.base = np.ascontiguousarray(base, np.float32)


def _targets(nv, lists, deltas):
    ts = np.zeros(len(lists) + 1, np.uint32)
    ts[1:] = np.cumsum([len(v) for v in lists])
    return dict(ts=ts, vertex=np.concatenate(lists).astype(np.uint32), dP=np.ascontiguousarray(np.concatenate(deltas), np.float32),
                dN=None, dB=None, pivot=0, num_vertices=nv, num_targets=len(lists))


def morph_rigs(p0):
    """Targets in which vertex v has MORPH_ENTRIES[v % 6] entries (target t holds the vertices with more than t), with
    weights that are all non-zero, with zeros of both signs on a base that has -0.0 coordinates (a skipped target keeps the
    bits), a dense target that cancels the base exactly, one that flattens it onto z = 0 at weight 1, and the first
    followed by the skin that scales z to zero."""
    nv = len(p0)
    lo, hi = _box(p0)
    ctr, ext = 0.5 * (lo + hi), float(np.max(hi - lo))
    rng = np.random.default_rng(21)
    per = np.array(MORPH_ENTRIES)[np.arange(nv) % 6]
    lists = [np.flatnonzero(per > t) for t in range(9)]
    tg = _targets(nv, lists, [(rng.normal(size=(len(v), 3)) * 0.01 * ext) for v in lists])
    w_all = np.array([1.25, -0.5, 0.75, 2.0, -1.5, 0.25, 1.0, -0.125, 0.5], np.float32)
    w_zero = np.array([-0.0, 1.25, 0.0, 2.0, -0.0, 0.0, -0.0, 0.0, 0.5], np.float32)
    base_nz = p0.copy()
    base_nz[np.random.default_rng(22).random(p0.shape) < 0.05] = np.float32(-0.0)
    base_nz[0, 0] = np.float32(-0.0)
    entries = lambda q: len(set(np.bincount(tg["vertex"], minlength=nv))) == 6 and np.isfinite(q).all() and not np.array_equal(q, p0)
    rigs = [MorphRig("entries", tg, w_all, p0, "bits", entries),
            MorphRig("zero_weights", tg, w_zero, base_nz, "bits",
                     # (the vertices with one entry are touched by a skipped target alone: they keep their bits, -0.0 among them)
                     lambda q: (np.array_equal(q[per == 1].view(np.uint32), base_nz[per == 1].view(np.uint32))
                                and int(((base_nz[per == 1] == 0) & np.signbit(base_nz[per == 1])).sum()) > 20
                                and not np.array_equal(q[per > 1], base_nz[per > 1])))]
    dense = [np.arange(nv)]
    rigs.append(MorphRig("cancelling", _targets(nv, dense, [-p0.astype(np.float64)]), [1.0], p0, "class",
                         lambda q: (q == 0).all() and not np.signbit(q).any()))
    dz = np.zeros((nv, 3))
    dz[:, 2] = -p0[:, 2].astype(np.float64)
    rigs.append(MorphRig("flatten", _targets(nv, dense, [dz]), [1.0], p0, "bits",
                         lambda q: (q[:, 2] == 0).all() and np.array_equal(q[:, 0:2], p0[:, 0:2])))
    one = np.zeros((nv, 4), np.float32)
    one[:, 0] = 1.0
    ids = np.zeros((nv, 4), np.uint16)
    ids[:, 0] = 1
    skin = dict(W=one, I=ids, bones=np.ascontiguousarray(np.stack([_bone(), _bone((1, 1, 0), ctr)]), np.float32))
    rigs.append(MorphRig("entries_then_zero_z_skin", tg, w_all, p0, "bits", lambda q: (q[:, 2] == q[0, 2]).all() and np.isfinite(q).all(), skin))
    return rigs


# ---- a float64 reading of both deformers: the same formulas from the fp32 inputs, no rounding in between ----------------
def skin_f64(p, W, I, bones):
    m = bones.astype(np.float64).reshape(-1, 4, 4)
    w = W.astype(np.float64)
    with np.errstate(all="ignore"):
        B = sum(m[I[:, k].astype(np.int64)] * w[:, k, None, None] for k in range(4))
        out = np.einsum("vr,vrc->vc", np.concatenate([p.astype(np.float64), np.ones((len(p), 1))], axis=1), B)[:, 0:3]
    static = (W == 0).all(axis=1)
    out[static] = p[static]
    return out


def morph_f64(base, tg, weights):
    x = base.astype(np.float64).copy()
    for t in range(tg["num_targets"]):
        a, b = int(tg["ts"][t]), int(tg["ts"][t + 1])
        if a < b and weights[t] != 0:
            x[tg["vertex"][a:b]] += float(weights[t]) * tg["dP"][a:b].astype(np.float64)
    return x


def deviation(got, want64):
    """largest |got - want64| over the largest |want64| (norm-wise: a collapsed coordinate has nothing of its own to scale by)"""
    with np.errstate(all="ignore"):
        return float(np.abs(got.astype(np.float64) - want64).max() / max(float(np.abs(want64).max()), 1e-300))


# Measured deviation of the fp32 restatement (== bdpt_host_skin / bdpt_host_morph, bit for bit) from the float64 reading on
# the atrium, per family; the tests allow four times as much.  The cancelling and overflowing families are compared by
# class only: their fp32 result is exactly zero, or not finite.
# (0: the fp32 arithmetic is exact there — a scale of 0, 1 or -1 about a centre whose coordinate is 0 or is added once.)
RIG_DEVIATION = {
    "skin zero_z": 0.0, "skin zero_yz": 0.0, "skin zero_xyz": 0.0, "skin mirror_x": 0.0, "skin far_1e5": 4.167e-08,
    "skin subnormal_weights": 4.671e-07, "skin palette_1_zero_z": 0.0, "skin palette_64_zero_z": 0.0, "skin palette_65_zero_z": 0.0,
    "morph entries": 1.436e-07, "morph zero_weights": 8.416e-08, "morph flatten": 0.0, "morph entries_then_zero_z_skin": 1.436e-07,
}
