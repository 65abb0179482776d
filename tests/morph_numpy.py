"""The morph-target arithmetic of include/bdpt.h "Morph targets" restated in numpy float32, and a seeded generator of
targets and weights for the morph tests.

Every operation below is an elementwise float32 numpy operation on arrays, one rounding each and never fused, in the
order the header fixes: x = base, then per target in ascending order np.where(w != 0, x + w * d, x); skin_numpy.skin
follows where there is a skin.  The library (csrc/morph.h, compiled without contraction) must give the same bits.

What the generator covers.  One set of targets cannot hold a dense target and vertices that are in no target at once, so
the cases are spread over the target counts the tests use:
  T = 1     one sparse target over about a third of the vertices: vertices in none, entries on vertex 0 and the last;
  T = 3     a dense target (every vertex), a sparse target, an empty target;
  T >= 4    a dense target, an empty target, sparse targets of about `sparse` vertices each.
In every set one vertex (`pivot`) is in every non-empty target, and vertex 0 and the last vertex are in the first sparse
target.  dense=False leaves the dense target out (it becomes one more sparse one), so that vertices in none remain."""
import ctypes as C

import numpy as np

import skin_numpy as sn

F = np.float32


def make_targets(seed, num_vertices, num_targets, normals=True, bitangents=True, dense=None, sparse=64, candidates=None,
                 scale=0.01, unit_scale=0.1):
    """dict of ts (T + 1, uint32), vertex (entries, uint32), dP, dN, dB (entries x 3 float32; dN / dB None when not asked
    for), pivot.  candidates: the vertices sparse targets draw from (default: all); scale: the size of position deltas,
    unit_scale: of normal and bitangent deltas."""
    rng = np.random.default_rng(seed)
    nv, T = int(num_vertices), int(num_targets)
    cand = np.arange(nv) if candidates is None else np.asarray(candidates)
    if dense is None:
        dense = T >= 2
    pivot = int(cand[len(cand) // 2])
    ends = [int(cand[0]), int(cand[-1])]
    lists = []
    first_sparse = True
    for t in range(T):
        if t == 0 and dense and candidates is None:
            lists.append(np.arange(nv))
        elif (t == 1 and T >= 3) or (t == 2 and T >= 1024):
            lists.append(np.zeros(0, np.int64))  # an empty target
        else:
            k = min(len(cand), max(1, len(cand) // 3) if T == 1 else sparse)
            v = list(rng.choice(cand, size=k, replace=False)) + [pivot]
            if first_sparse:
                v += ends
                first_sparse = False
            lists.append(np.unique(np.asarray(v, np.int64)))
    ts = np.zeros(T + 1, np.uint32)
    ts[1:] = np.cumsum([len(v) for v in lists])
    vertex = np.concatenate(lists).astype(np.uint32)
    ne = vertex.size
    delta = lambda s: (rng.normal(size=(ne, 3)) * s).astype(F)
    return dict(ts=ts, vertex=vertex, dP=delta(scale), dN=delta(unit_scale) if normals else None,
                dB=delta(unit_scale) if bitangents else None, pivot=pivot, num_vertices=nv, num_targets=T)


def make_weights(seed, num_targets):
    """(T,) float32: zeros of both signs, negatives and values above 1 among them"""
    T = int(num_targets)
    if T == 1:
        return np.array([[1.25], [-0.5]][seed % 2], F)
    if T == 3:
        return np.array([[-0.75, 1.5, -0.0], [0.0, 0.625, 1.25]][seed % 2], F)
    rng = np.random.default_rng(seed)
    w = rng.uniform(-1.0, 2.0, T).astype(F)
    zero = rng.random(T) < 0.3
    w[zero] = np.where(rng.random(int(zero.sum())) < 0.5, F(0.0), F(-0.0))
    w[0] = F([-0.75, 1.5][seed % 2])  # (the dense target moves every vertex)
    w[T - 1], w[T - 2], w[T - 3], w[T - 4] = F(0.0), F(-0.0), F(-0.25), F(1.75)
    return w


def with_negative_zeros(a, seed, share=0.05):
    """a copy of the (nv, 3) array with -0.0 in a share of its components, vertex 0's first among them"""
    rng = np.random.default_rng(seed)
    out = np.ascontiguousarray(a, F).copy()
    out[rng.random(out.shape) < share] = F(-0.0)
    out[0, 0] = F(-0.0)
    return out


def morph_stream(base, tg, d, weights):
    """One stream: x = base; per target in ascending order, on its vertices, np.where(w != 0, x + w * d, x)"""
    x = np.ascontiguousarray(base, F).reshape(-1, 3).copy()
    if d is None:
        return x
    ts, vertex = tg["ts"], tg["vertex"]
    for t in range(len(ts) - 1):
        a, b = int(ts[t]), int(ts[t + 1])
        if a == b:
            continue
        idx = vertex[a:b]
        w = F(weights[t])
        cur = x[idx]
        term = w * d[a:b]
        assert term.dtype == F
        x[idx] = np.where(w != 0, cur + term, cur)
    assert x.dtype == F
    return x


def morph(tg, weights, P, N=None, B=None, rig=None, bones=None, normal_bones=None):
    """(positions', normals' or None, bitangents' or None): the morphed base, skinned by skin_numpy.skin where `rig`
    (a dict with W and I) is given"""
    p = morph_stream(P, tg, tg["dP"], weights)
    n = None if N is None else morph_stream(N, tg, tg["dN"], weights)
    b = None if B is None else morph_stream(B, tg, tg["dB"], weights)
    if rig is None:
        return p, n, b
    return sn.skin(p, rig["W"], rig["I"], bones, normal_bones, n, b)


def morph_desc(abi, tg, P=None, N=None, B=None):
    """A bdpt_morph_desc over the arrays (which the caller keeps alive); P, N, B: the base, None with a skin"""
    d = abi.MorphDesc()
    d.numVertices, d.numTargets = tg["num_vertices"], tg["num_targets"]
    ptr = lambda a: None if a is None else a.ctypes.data
    d.targetStart, d.vertex = ptr(tg["ts"]), ptr(tg["vertex"])
    d.dPositions, d.dNormals, d.dBitangents = ptr(tg["dP"]), ptr(tg["dN"]), ptr(tg["dB"])
    d.positions, d.normals, d.bitangents = ptr(P), ptr(N), ptr(B)
    return d


def only(tg, normals=True, bitangents=True):
    """the same targets without their normal / bitangent deltas"""
    out = dict(tg)
    if not normals:
        out["dN"] = None
    if not bitangents:
        out["dB"] = None
    return out


def host_morph(lib, abi, tg, weights, P, N=None, B=None, rig=None, bones=None, normal_bones=None):
    """bdpt_host_morph: (rc, positions', normals' or None, bitangents' or None).  With `rig` the base P, N, B is the skin
    desc's rest pose, else the morph desc's own."""
    ptr = lambda a: None if a is None else a.ctypes.data
    if rig is not None:
        sd = sn.skin_desc(abi, P, rig["W"], rig["I"], bones.shape[0], N, B)
        md = morph_desc(abi, tg)
        skin = C.byref(sd)
    else:
        md = morph_desc(abi, tg, P, N, B)
        skin = None
    op = np.full_like(P, 7.0)
    on = None if N is None else np.full_like(N, 7.0)
    ob = None if B is None else np.full_like(B, 7.0)
    rc = lib.bdpt_host_morph(C.byref(md), skin, ptr(weights), ptr(bones), ptr(normal_bones if N is not None else None), ptr(op), ptr(on),
                             ptr(ob))
    return rc, op, on, ob


def set_morph(ctx, tg, P=None, N=None, B=None):
    ctx.set_morph(tg["ts"], tg["vertex"], tg["dP"], tg["dN"], tg["dB"], P, N, B)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)
