"""Host-side tests of morph targets (include/bdpt.h "Morph targets"): bdpt_host_morph — the per-vertex functions the device
kernel runs (csrc/morph.h, csrc/skin.h), compiled for the CPU — against the numpy float32 restatement of
tests/morph_numpy.py, bit for bit; struct layouts; error codes; and the checks and the host / device path choice of
Context.set_morph / update_morphed.  No GPU: the kernel is compared with the same restatement by
tests/test_gpu_morph.py."""
import ctypes as C

import numpy as np
import pytest

import binding_fakes as fakes
import morph_numpy as mn
import skin_numpy as sn
from binding_fakes import RecordingLib, context_without_device
from test_skinning_cpu import _soup_rig


@pytest.fixture(scope="module")
def rig(pkg):
    """A soup of 24 003 vertices (no multiple of 64) with a 5-bone rig, base components that are -0.0, and one pose; made
    once and left unchanged"""
    r = _soup_rig(pkg, 5, 8001, 5)
    for k in "PNB":
        r[k] = mn.with_negative_zeros(r[k], 3 + ord(k))
    r["bones"], r["nbones"] = sn.make_pose(9, 5, r["pivot"], r["extent"])
    return r


def _streams(r, streams):
    return r["P"], (r["N"] if "n" in streams else None), (r["B"] if "b" in streams else None)


def _assert_matches(lib, abi, r, tg, w, streams, skinned):
    P, N, B = _streams(r, streams)
    tg = mn.only(tg, N is not None, B is not None)
    kw = dict(rig=r, bones=r["bones"], normal_bones=r["nbones"]) if skinned else {}
    rc, op, on, ob = mn.host_morph(lib, abi, tg, w, P, N, B, **kw)
    assert rc == 0, (streams, skinned)
    ep, en, eb = mn.morph(tg, w, P, N, B, **kw)
    assert np.array_equal(mn.bits(op), mn.bits(ep)), f"{streams} skinned={skinned}: {(mn.bits(op) != mn.bits(ep)).any(axis=1).sum()} positions differ"
    assert (on is None) == (N is None) and (ob is None) == (B is None)
    if N is not None:
        assert np.array_equal(mn.bits(on), mn.bits(en)), (streams, skinned)
    if B is not None:
        assert np.array_equal(mn.bits(ob), mn.bits(eb)), (streams, skinned)
    return op, on, ob


@pytest.mark.parametrize("num_targets", [1, 3, 1024])
def test_host_morph_equals_the_restatement(pkg, rig, num_targets):
    """1, 3 and 1024 targets, with and without a skin desc, every subset of streams, two weight vectors."""
    lib = pkg.load_library()
    nv = rig["P"].shape[0]
    tg = mn.make_targets(20 + num_targets, nv, num_targets)
    counts = np.bincount(tg["vertex"], minlength=nv)
    assert counts[tg["pivot"]] == (np.diff(tg["ts"].astype(np.int64)) > 0).sum() and counts[0] and counts[nv - 1]
    if num_targets == 1:
        assert (counts == 0).any()
    else:
        assert tg["ts"][1] == nv and (np.diff(tg["ts"].astype(np.int64)) == 0).any()  # a dense target, an empty one
    for seed in (0, 1):
        w = mn.make_weights(seed, num_targets)
        for skinned in (False, True):
            for streams in ("p", "pb", "pn", "pnb"):
                op, on, ob = _assert_matches(lib, pkg.abi, rig, tg, w, streams, skinned)
    if num_targets > 3:
        assert (w == 0).any() and np.signbit(w[w == 0]).any() and not np.signbit(w[w == 0]).all() and (w < 0).any() and (w > 1).any()
    assert not np.array_equal(op, rig["P"])
    # a base stream without deltas: normals are skinned (or copied) but not morphed
    for skinned in (False, True):
        P, N, B = _streams(rig, "pnb")
        t2 = mn.only(tg, normals=False)
        kw = dict(rig=rig, bones=rig["bones"], normal_bones=rig["nbones"]) if skinned else {}
        rc, op, on, ob = mn.host_morph(lib, pkg.abi, t2, w, P, N, B, **kw)
        ep, en, eb = mn.morph(t2, w, P, N, B, **kw)
        assert rc == 0 and all(np.array_equal(mn.bits(g), mn.bits(e)) for g, e in ((op, ep), (on, en), (ob, eb)))
        if not skinned:
            assert np.array_equal(mn.bits(on), mn.bits(N))


def test_zero_weights_return_the_base_bits(pkg, rig):
    """All weights zero, of either sign: the base bit for bit, its -0.0 components included; with a skin desc, what
    bdpt_host_skin gives."""
    lib = pkg.load_library()
    nv = rig["P"].shape[0]
    tg = mn.make_targets(7, nv, 3)
    P, N, B = _streams(rig, "pnb")
    assert np.signbit(P[P == 0]).any() and np.signbit(P[0, 0])
    w = np.array([0.0, -0.0, -0.0], np.float32)
    rc, op, on, ob = mn.host_morph(lib, pkg.abi, tg, w, P, N, B)
    assert rc == 0
    for out, base in ((op, P), (on, N), (ob, B)):
        assert np.array_equal(mn.bits(out), mn.bits(base))
    rc, op, on, ob = mn.host_morph(lib, pkg.abi, tg, w, P, N, B, rig=rig, bones=rig["bones"], normal_bones=rig["nbones"])
    rc2, sp, sn_, sb = sn.host_skin(lib, pkg.abi, P, rig["W"], rig["I"], rig["bones"], rig["nbones"], N, B)
    assert rc == 0 and rc2 == 0
    for out, ref in ((op, sp), (on, sn_), (ob, sb)):
        assert np.array_equal(mn.bits(out), mn.bits(ref))
    # one non-zero weight on a sparse target: vertices outside it still keep their bits
    w[2] = 1.5
    rc, op, _, _ = mn.host_morph(lib, pkg.abi, tg, w, P, N, B)
    outside = np.ones(nv, bool)
    outside[tg["vertex"][tg["ts"][2]:tg["ts"][3]]] = False
    assert 0 < (~outside).sum() < 100
    assert rc == 0 and np.array_equal(mn.bits(op[outside]), mn.bits(P[outside])) and not np.array_equal(op[~outside], P[~outside])


def test_morph_structs_and_constants(pkg):
    a = pkg.abi
    lay = fakes.header_layout({"bdpt_morph_desc": [f for f, _ in a.MorphDesc._fields_], "bdpt_morph_update": [f for f, _ in a.MorphUpdate._fields_]},
                              {"MAX": ["BDPT_MAX_MORPH_TARGETS"]})
    for cname, cls in (("bdpt_morph_desc", a.MorphDesc), ("bdpt_morph_update", a.MorphUpdate)):
        assert int(lay[cname]) == C.sizeof(cls)
        for f, _ in cls._fields_:
            assert int(lay[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)
    assert C.sizeof(a.MorphDesc) == 80 and C.sizeof(a.MorphUpdate) == 48
    assert int(lay["MAX"]) == a.MAX_MORPH_TARGETS == 1024
    assert (a.MORPH_PATH_AUTO, a.MORPH_PATH_GLOBAL, a.MORPH_PATH_LDS) == (a.SKIN_PATH_AUTO, a.SKIN_PATH_GLOBAL, a.SKIN_PATH_LDS) == (0, 1, 2)
    lib = pkg.load_library()
    for name in ("bdpt_set_morph", "bdpt_update_morphed", "bdpt_morphed_buffers", "bdpt_host_morph", "bdpt_test_morph_kernel"):
        assert hasattr(lib, name) and name in a.PROTOTYPES
    assert a.PROTOTYPES["bdpt_set_morph"] == (C.c_int, [C.c_void_p, C.POINTER(a.MorphDesc)])
    assert a.PROTOTYPES["bdpt_update_morphed"] == (C.c_int, [C.c_void_p, C.POINTER(a.MorphUpdate), C.c_void_p])
    assert len(a.PROTOTYPES["bdpt_host_morph"][1]) == 8 and len(a.PROTOTYPES["bdpt_morphed_buffers"][1]) == 4


def test_host_morph_error_codes(pkg):
    """Every desc check of include/bdpt.h "Morph targets" that needs no context."""
    lib, a = pkg.load_library(), pkg.abi
    r = _soup_rig(pkg, 8, 40, 4, static_share=0.3)
    P, N, B = r["P"], r["N"], r["B"]
    nv = P.shape[0]
    bones, nbones = sn.make_pose(4, 4, r["pivot"], r["extent"])
    tg = mn.make_targets(1, nv, 3, sparse=10)
    w = mn.make_weights(0, 3)
    out = np.zeros_like(P)
    ptr = lambda x: None if x is None else x.ctypes.data

    def call(md, sd=None, w_=w, bones_=None, nb=None, op=out, on=out, ob=out):
        return lib.bdpt_host_morph(None if md is None else C.byref(md), None if sd is None else C.byref(sd), ptr(w_), ptr(bones_), ptr(nb),
                                   ptr(op), ptr(on), ptr(ob))

    good = lambda **kw: mn.morph_desc(a, dict(tg, **kw), P, N, B)
    skin = lambda n=N, b=B: sn.skin_desc(a, P, r["W"], r["I"], 4, n, b)
    on_skin = lambda **kw: mn.morph_desc(a, dict(tg, **kw))
    assert call(good()) == 0
    assert call(on_skin(), skin(), bones_=bones, nb=nbones) == 0
    # NULL arguments
    assert call(None) == -1 and call(good(), w_=None) == -1 and call(good(), op=None) == -1
    assert call(good(), on=None) == -1 and call(good(), ob=None) == -1
    assert call(mn.morph_desc(a, mn.only(tg, False, False), P), on=None, ob=None) == 0  # positions alone need neither
    for field in ("targetStart", "vertex", "dPositions"):
        d = good()
        setattr(d, field, None)
        assert call(d) == -1, field
    # counts, reserved
    d = good()
    d.numTargets = 0
    assert call(d) == -1
    d = good()
    d.numTargets = 1025
    assert call(d) == -5
    d = good()
    d.reserved[1] = 1
    assert call(d) == -1
    # targetStart
    ts = tg["ts"].copy()
    ts[0] = 1
    assert call(good(ts=ts)) == -1
    ts = tg["ts"].copy()
    ts[1], ts[2] = ts[2], ts[1] - 1
    assert ts[2] < ts[1] and call(good(ts=ts)) == -1
    big = np.array([0, 1 << 31], np.uint32)  # 2^31 entries: refused before an entry is read
    d = mn.morph_desc(a, dict(tg, ts=big, num_targets=1), P, N, B)
    assert call(d) == -5
    # vertex ids
    a0, a1 = int(tg["ts"][0]), int(tg["ts"][1])
    assert a1 - a0 == nv
    vx = tg["vertex"].copy()
    vx[a1 - 1] = nv
    assert call(good(vertex=vx)) == -1
    vx = tg["vertex"].copy()
    vx[a0 + 3] = vx[a0 + 2]  # twice the same id
    assert call(good(vertex=vx)) == -1
    vx = tg["vertex"].copy()
    vx[a0 + 2], vx[a0 + 3] = vx[a0 + 3], vx[a0 + 2]  # descending
    assert call(good(vertex=vx)) == -1
    # finiteness: deltas, base values, weights
    for bad in (np.nan, np.inf):
        for key in ("dP", "dN", "dB"):
            x = tg[key].copy()
            x[5, 1] = bad
            assert call(good(**{key: x})) == -1, key
        for k, base in enumerate((P, N, B)):
            x = base.copy()
            x[3, 2] = bad
            args = [P, N, B]
            args[k] = x
            assert call(mn.morph_desc(a, tg, *args)) == -1, k
        w2 = w.copy()
        w2[2] = bad
        assert call(good(), w_=w2) == -1
    # base pose: given with a skin, missing without one; deltas for a stream the base lacks
    assert call(good(), skin(), bones_=bones, nb=nbones) == -1
    assert call(mn.morph_desc(a, tg, None, N, B)) == -1
    assert call(mn.morph_desc(a, tg, P, None, B), on=None) == -1 and call(mn.morph_desc(a, tg, P, N, None), ob=None) == -1
    assert call(mn.morph_desc(a, mn.only(tg, normals=False), P, None, B), on=None) == 0
    assert call(on_skin(), skin(n=None), bones_=bones) == -1 and call(on_skin(), skin(b=None), bones_=bones, nb=nbones) == -1
    assert call(mn.morph_desc(a, mn.only(tg, normals=False)), skin(n=None), bones_=bones) == 0
    # palettes missing with a skin, or given without one; the skin's own checks and size
    assert call(on_skin(), skin()) == -1 and call(on_skin(), skin(), bones_=bones) == -1
    assert call(good(), bones_=bones) == -1 and call(good(), nb=nbones) == -1
    sd = skin()
    sd.numVertices = nv - 1
    assert call(on_skin(), sd, bones_=bones, nb=nbones) == -1
    sd = skin()
    sd.numBones = 1025
    assert call(on_skin(), sd, bones_=bones, nb=nbones) == -5


def _context_without_device(pkg, device=0):
    """a Context whose library records what bdpt_update_morphed (.calls) and bdpt_set_morph (.morphs) were handed"""
    lib = RecordingLib({"bdpt_update_morphed": lambda g, stream: (g.memory, g.weights, g.bones, g.normalBones, g.numTargets, g.numBones, g.flags)})
    lib.morphs = []

    def set_morph(h, d):
        o = None if d is None else d._obj
        lib.morphs.append(None if o is None else (o.numVertices, o.numTargets, bool(o.dNormals), bool(o.dBitangents), bool(o.positions),
                                                  bool(o.normals), bool(o.bitangents)))
        return 0

    lib.bdpt_set_morph = set_morph
    return context_without_device(pkg, lib, device)


def test_update_morphed_picks_the_host_or_the_device_path(pkg):
    """numpy arrays and CPU tensors go down the host path, GPU tensors down the device path; mixed inputs, another GPU's
    memory and bad shapes are refused before anything reaches the library."""
    import torch
    ctx = _context_without_device(pkg)
    w = np.array([0.5, 0.0, 1.5], np.float32)
    m = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (2, 1))
    ctx.update_morphed(w)
    assert ctx._lib.calls[-1] == (pkg.abi.MEMORY_HOST, w.ctypes.data, None, None, 3, 0, 0)
    ctx.update_morphed(torch.from_numpy(w.copy()), torch.from_numpy(m.copy()), torch.from_numpy(m.copy()), keep_light_maps=True)
    mem, pw, pb, pn, nt, nb, flags = ctx._lib.calls[-1]
    assert mem == pkg.abi.MEMORY_HOST and pw and pb and pn and (nt, nb) == (3, 2) and flags == pkg.abi.UPDATE_KEEP_LIGHT_MAPS
    calls = len(ctx._lib.calls)
    with pytest.raises(pkg.BdptError):
        ctx.update_morphed(None)
    with pytest.raises(pkg.BdptError):
        ctx.update_morphed(w, m, m[:1])  # palettes of two sizes
    with pytest.raises(pkg.BdptError):
        ctx.update_morphed(w, np.ones(20, np.float32))  # not numBones x 16
    with pytest.raises(pkg.BdptError):
        ctx.update_morphed(w, None, m)  # inverse transposes without bones
    with pytest.raises(pkg.BdptError):
        ctx.update_morphed(np.zeros(0, np.float32))

    def gpu(shape, index=0, contiguous=True, ptr=0x2000):
        return fakes.FakeGpuTensor(shape, torch.float32, index, contiguous, ptr=ptr)

    with pytest.raises(pkg.BdptError):
        ctx.update_morphed(gpu((3,), index=1))  # another GPU's memory
    with pytest.raises(pkg.BdptError):
        ctx.update_morphed(gpu((3,)), m)  # GPU weights, host bones
    with pytest.raises(pkg.BdptError):
        ctx.update_morphed(w, gpu((2, 16)))  # host weights, GPU bones
    with pytest.raises(pkg.BdptError):
        ctx.update_morphed(gpu((3,), contiguous=False))
    assert len(ctx._lib.calls) == calls
    ctx.update_morphed(gpu((3,), ptr=0x1000), gpu((2, 16)), gpu((2, 16), ptr=0x3000))
    assert ctx._lib.calls[-1] == (pkg.abi.MEMORY_DEVICE, 0x1000, 0x2000, 0x3000, 3, 2, 0)
    ctx.update_morphed(gpu((3,), ptr=0x1000))
    assert ctx._lib.calls[-1] == (pkg.abi.MEMORY_DEVICE, 0x1000, None, None, 3, 0, 0)


def test_set_morph_binding_checks_shapes(pkg):
    ctx = _context_without_device(pkg)
    P = np.zeros((5, 3), np.float32)
    ts = np.array([0, 2, 2, 3], np.uint32)
    vx = np.array([1, 4, 0], np.uint32)
    d = np.ones((3, 3), np.float32)
    ctx.set_morph(ts, vx, d, d_normals=d, positions=P, normals=P)
    assert ctx._lib.morphs[-1] == (5, 3, True, False, True, True, False)
    ctx._skin_vertices = 7  # (a skinned context: no base arrays, the vertex count is the skin's)
    ctx.set_morph(ts, vx, d)
    assert ctx._lib.morphs[-1] == (7, 3, False, False, False, False, False)
    n = len(ctx._lib.morphs)
    with pytest.raises(pkg.BdptError):
        ctx.set_morph(ts, vx[:2], d, positions=P)  # target_start does not end at the entry count
    with pytest.raises(pkg.BdptError):
        ctx.set_morph(ts, vx, d[:2], positions=P)
    with pytest.raises(pkg.BdptError):
        ctx.set_morph(ts, vx, d, d_bitangents=d[:1], positions=P, bitangents=P)
    with pytest.raises(pkg.BdptError):
        ctx.set_morph(ts, vx, d, positions=P, normals=P[:4])
    with pytest.raises(pkg.BdptError):
        ctx.set_morph(ts, vx, d, normals=P)  # a base without positions
    with pytest.raises(pkg.BdptError):
        ctx.set_morph(ts[:1], vx[:0], d[:0], positions=P)  # no target
    assert len(ctx._lib.morphs) == n
    ctx.set_morph(None, None, None)
    assert ctx._lib.morphs[-1] is None
