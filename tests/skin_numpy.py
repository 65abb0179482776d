"""The skinning arithmetic of include/bdpt.h "Skinning" restated in numpy float32, and rigs for the skinning tests.

Every operation below is an elementwise float32 numpy operation on arrays, one rounding each and never fused, in the
order the header fixes; the library (csrc/skin.h, compiled without contraction) must give the same bits."""
import ctypes as C

import numpy as np

F = np.float32


def is_static(weights):
    """vertices whose four weights are all zero, of either sign"""
    return (np.asarray(weights, F).reshape(-1, 4) == 0).all(axis=1)


def _blend(mats, ids, w):
    """B[e] = ((M[i0][e]*w0 + M[i1][e]*w1) + M[i2][e]*w2) + M[i3][e]*w3 for every vertex: (nv, 16) float32"""
    m = np.ascontiguousarray(mats, F).reshape(-1, 16)
    g = [m[ids[:, k]] for k in range(4)]
    wk = [w[:, k:k + 1] for k in range(4)]
    b = ((g[0] * wk[0] + g[1] * wk[1]) + g[2] * wk[2]) + g[3] * wk[3]
    assert b.dtype == F
    return b


def _mul3(v, b, translate):
    out = np.empty((v.shape[0], 3), F)
    for c in range(3):
        s = (v[:, 0] * b[:, c] + v[:, 1] * b[:, 4 + c]) + v[:, 2] * b[:, 8 + c]
        out[:, c] = s + b[:, 12 + c] if translate else s
    return out


def skin(positions, weights, ids, bones, normal_bones=None, normals=None, bitangents=None):
    """(positions', normals' or None, bitangents' or None); static vertices keep their rest values bit for bit and
    their ids are not read."""
    p = np.ascontiguousarray(positions, F).reshape(-1, 3)
    w = np.ascontiguousarray(weights, F).reshape(-1, 4)
    st = is_static(w)
    i = np.where(st[:, None], 0, np.asarray(ids).reshape(-1, 4).astype(np.int64))
    b = _blend(bones, i, w)
    keep = lambda rest, moved: np.where(st[:, None], rest, moved).astype(F)
    out_p = keep(p, _mul3(p, b, True))
    out_n = out_b = None
    if normals is not None:
        n = np.ascontiguousarray(normals, F).reshape(-1, 3)
        out_n = keep(n, _mul3(n, _blend(normal_bones, i, w), False))
    if bitangents is not None:
        t = np.ascontiguousarray(bitangents, F).reshape(-1, 3)
        out_b = keep(t, _mul3(t, b, False))
    return out_p, out_n, out_b


def make_rig(seed, num_vertices, num_bones, static_share=0.25, normalised=True, static_mask=None):
    """(weights (nv, 4) float32, ids (nv, 4) uint16): one to four non-zero weights per vertex (the rest exactly zero, now
    and then -0.0), ids anywhere in the palette; a share of static vertices (all weights zero) whose ids are 0xFFFF,
    beyond any palette.  static_mask: exactly these vertices are static instead of a random share."""
    rng = np.random.default_rng(seed)
    nv = num_vertices
    ids = rng.integers(0, num_bones, (nv, 4)).astype(np.uint16)
    w = rng.uniform(0.05, 1.0, (nv, 4))
    used = rng.integers(1, 5, nv)
    w[np.arange(4)[None, :] >= used[:, None]] = 0.0
    if normalised:
        w /= w.sum(axis=1, keepdims=True)
    else:
        w *= rng.uniform(0.6, 1.3, (nv, 1))  # weights that do not sum to 1
    w = w.astype(F)
    w[(w == 0) & (rng.random((nv, 4)) < 0.2)] = F(-0.0)
    st = rng.random(nv) < static_share if static_mask is None else np.asarray(static_mask, bool)
    w[st] = np.where(rng.random((int(st.sum()), 4)) < 0.5, F(0.0), F(-0.0))
    ids[st] = 0xFFFF
    return w, ids


def make_pose(seed, num_bones, pivot, extent, angle=0.15, shift=0.01, scale=0.05):
    """(bones, normal_bones): (nb, 16) float32 each, m[4r+c] for row vectors (pos' = (pos, 1) . M, translation in floats
    12..14).  Every bone: a proper rotation by up to `angle` radians about `pivot`, a non-uniform scale within
    1 +- `scale`, a translation of up to `shift` * extent.  normal_bones: the inverse transposes (float64, rounded once)."""
    rng = np.random.default_rng(seed)
    pivot = np.asarray(pivot, np.float64)
    bones = np.zeros((num_bones, 4, 4))
    for k in range(num_bones):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        a = rng.uniform(-angle, angle)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
        assert np.linalg.det(R) > 0.999
        A = np.diag(rng.uniform(1 - scale, 1 + scale, 3)) @ R.T  # row-vector convention: p' = p . A
        t = rng.uniform(-shift, shift, 3) * extent
        bones[k, :3, :3] = A
        bones[k, 3, :3] = pivot - pivot @ A + t
        bones[k, 3, 3] = 1.0
    nbones = np.transpose(np.linalg.inv(bones), (0, 2, 1))
    return bones.reshape(num_bones, 16).astype(F), nbones.reshape(num_bones, 16).astype(F)


def scene_rig(desc, seed, num_bones, **kw):
    """Rest arrays of a scene description and a rig for it: dict of P, N, B (None without bitangents), W, I, pivot, extent"""
    nv = int(desc.numVertices)
    v3 = lambda ptr: np.ctypeslib.as_array(ptr, shape=(nv, 3)).astype(F).copy()
    P = v3(desc.positions)
    w, ids = make_rig(seed, nv, num_bones, **kw)
    lo, hi = P.min(axis=0), P.max(axis=0)
    return dict(P=P, N=v3(desc.normals), B=v3(desc.bitangents) if desc.bitangents else None, W=w, I=ids,
                pivot=(lo + hi) * 0.5, extent=float(np.max(hi - lo)))


def skin_desc(abi, P, W, I, num_bones, N=None, B=None):
    """A bdpt_skin_desc over the arrays (which the caller keeps alive)"""
    d = abi.SkinDesc()
    d.numVertices, d.numBones = P.shape[0], num_bones
    d.positions, d.boneWeights, d.boneIds = P.ctypes.data, W.ctypes.data, I.ctypes.data
    d.normals = None if N is None else N.ctypes.data
    d.bitangents = None if B is None else B.ctypes.data
    return d


def host_skin(lib, abi, P, W, I, bones, nbones=None, N=None, B=None):
    """bdpt_host_skin on the arrays: (rc, positions', normals' or None, bitangents' or None)"""
    d = skin_desc(abi, P, W, I, bones.shape[0], N, B)
    op = np.full_like(P, 7.0)
    on = None if N is None else np.full_like(N, 7.0)
    ob = None if B is None else np.full_like(B, 7.0)
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = lib.bdpt_host_skin(C.byref(d), ptr(bones), ptr(nbones), ptr(op), ptr(on), ptr(ob))
    return rc, op, on, ob


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)
