"""CPU checks of the surface queries' interface (bdpt_camera_rays, bdpt_shade_hits, bdpt_bsdf_query): the ctypes structures
against include/bdpt.h, and the Python binding's argument checks against a fake library, so that nothing a GPU would need
is involved."""
import ctypes as C

import numpy as np
import pytest

from binding_fakes import FakeGpuTensor, RecordingLib, _FakeOut, _NullContext, context_without_device, header_layout

STRUCTS = {
    "bdpt_surface": ("Surface", ["posW", "dist", "N", "linearRoughness", "V", "IoR", "diffuse", "opacity", "specular", "material",
                                 "emissive", "prim"]),
    "bdpt_shade_desc": ("ShadeDesc", ["rays", "hits", "numHits", "flags", "numHitsDevice", "surfaces"]),
    "bdpt_bsdf_sample": ("BsdfSample", ["dir", "pdf", "weight", "specular"]),
    "bdpt_bsdf_desc": ("BsdfDesc", ["surfaces", "num", "mode", "numDevice", "matIndex", "flags", "seeds", "samples", "dirs",
                                    "values"]),
}


def test_surface_structs_match_the_header(pkg):
    a = pkg.abi
    lay = header_layout({c: f for c, (_, f) in STRUCTS.items()}, {"consts": ["BDPT_SHADE_NORMAL_MAP", "BDPT_BSDF_SAMPLE", "BDPT_BSDF_EVAL"]})
    assert int(lay["bdpt_surface"]) == C.sizeof(a.Surface) == 96
    assert int(lay["bdpt_bsdf_sample"]) == C.sizeof(a.BsdfSample) == 32
    for cname, (pyname, fields) in STRUCTS.items():
        cls = getattr(a, pyname)
        assert int(lay[cname]) == C.sizeof(cls), cname
        assert [n for n, _ in cls._fields_] == fields, cname
        for name in fields:
            assert int(lay[f"{cname}.{name}"]) == getattr(cls, name).offset, (cname, name)
    assert lay["consts"] == f"{a.SHADE_NORMAL_MAP} {a.BSDF_SAMPLE} {a.BSDF_EVAL}"
    for n in ("bdpt_camera_rays", "bdpt_shade_hits", "bdpt_bsdf_query"):
        assert n in a.PROTOTYPES


def _context_without_device(pkg, device=0):
    """a Context whose library records what the three entry points are handed"""
    return context_without_device(pkg, RecordingLib({
        "bdpt_camera_rays": lambda gp, w, hh, rays, stream: dict(fn="camera_rays", w=w, h=hh, rays=rays),
        "bdpt_shade_hits": lambda d, stream: dict(fn="shade_hits", rays=d.rays, hits=d.hits, n=d.numHits, flags=d.flags,
                                                  count=d.numHitsDevice, out=d.surfaces),
        "bdpt_bsdf_query": lambda d, stream: dict(fn="bsdf", surfaces=d.surfaces, n=d.num, mode=d.mode, count=d.numDevice,
                                                  mat=d.matIndex, flags=d.flags, seeds=d.seeds, samples=d.samples, dirs=d.dirs,
                                                  values=d.values),
    }), device)


def test_good_calls_reach_the_library(pkg):
    import torch
    a = pkg.abi
    ctx = _context_without_device(pkg)
    rays, hits = FakeGpuTensor((64, 8), torch.float32, ptr=0x10000), FakeGpuTensor((64, 4), torch.int32, ptr=0x20000)
    surf = FakeGpuTensor((64, 24), torch.float32, ptr=0x30000)
    cnt = FakeGpuTensor((1,), torch.uint32, ptr=0x40000)
    ctx.shade_hits(rays, hits, out=surf, count=cnt)
    assert ctx._lib.calls[-1] == dict(fn="shade_hits", rays=0x10000, hits=0x20000, n=64, flags=a.SHADE_NORMAL_MAP, count=0x40000,
                                      out=0x30000)
    ctx.shade_hits(rays, FakeGpuTensor((64, 4), torch.float32, ptr=0x20000), normal_map=False,
                   out=FakeGpuTensor((64, 24), torch.int32, ptr=0x30000))
    assert ctx._lib.calls[-1]["flags"] == 0 and ctx._lib.calls[-1]["count"] is None
    seeds = FakeGpuTensor((64,), torch.uint32, ptr=0x50000)
    ctx.sample_bsdf(surf, seeds, mat_index=1, from_lobe=True, out=FakeGpuTensor((64, 8), torch.float32, ptr=0x60000))
    c = ctx._lib.calls[-1]
    assert (c["mode"], c["mat"], c["flags"], c["seeds"], c["samples"], c["surfaces"]) == (
        a.BSDF_SAMPLE, 1, a.PARAM_SPECULAR_FROM_LOBE, 0x50000, 0x60000, 0x30000)
    ctx.eval_bsdf(surf, FakeGpuTensor((64, 4), torch.float32, ptr=0x70000), out=FakeGpuTensor((64, 4), torch.float32, ptr=0x80000),
                  count=cnt)
    c = ctx._lib.calls[-1]
    assert (c["mode"], c["mat"], c["flags"], c["dirs"], c["values"], c["count"]) == (a.BSDF_EVAL, 0, 0, 0x70000, 0x80000, 0x40000)
    gp = a.GBufferParams()
    ctx.camera_rays(gp, 16, 9, out=FakeGpuTensor((144, 8), torch.float32, ptr=0x90000))
    assert ctx._lib.calls[-1] == dict(fn="camera_rays", w=16, h=9, rays=0x90000)


def test_bad_arguments_are_refused_before_the_library(pkg):
    import torch
    ctx = _context_without_device(pkg)
    rays, hits = FakeGpuTensor((64, 8), torch.float32), FakeGpuTensor((64, 4), torch.float32)
    surf, seeds = FakeGpuTensor((64, 24), torch.float32), FakeGpuTensor((64,), torch.int32)
    dirs = FakeGpuTensor((64, 4), torch.float32)
    gp = pkg.abi.GBufferParams()
    bad = [
        (ctx.shade_hits, dict(rays=FakeGpuTensor((64, 8), torch.float32, index=1), hits=hits)),       # another GPU
        (ctx.shade_hits, dict(rays=FakeGpuTensor((64, 8), torch.float64), hits=hits)),                # rays dtype
        (ctx.shade_hits, dict(rays=FakeGpuTensor((64, 7), torch.float32), hits=hits)),                # rays shape
        (ctx.shade_hits, dict(rays=rays, hits=FakeGpuTensor((63, 4), torch.float32))),                # lengths differ
        (ctx.shade_hits, dict(rays=rays, hits=FakeGpuTensor((64, 4), torch.float16))),                # hits dtype
        (ctx.shade_hits, dict(rays=rays, hits=FakeGpuTensor((64, 4), torch.float32, contiguous=False))),  # strides
        (ctx.shade_hits, dict(rays=rays, hits=hits, out=FakeGpuTensor((64, 23), torch.float32))),     # out shape
        (ctx.shade_hits, dict(rays=rays, hits=hits, out=FakeGpuTensor((64, 24), torch.float32, index=1))),  # out device
        (ctx.shade_hits, dict(rays=rays, hits=hits, count=FakeGpuTensor((1,), torch.int64))),         # count dtype
        (ctx.shade_hits, dict(rays=rays, hits=hits, count=FakeGpuTensor((2,), torch.int32))),         # count size
        (ctx.shade_hits, dict(rays=rays, hits=hits, count=torch.ones(1, dtype=torch.int32))),         # count on the host
        (ctx.shade_hits, dict(rays=rays, hits=np.zeros((64, 4), np.float32))),                        # GPU and host mixed
        (ctx.shade_hits, dict(rays=np.zeros((4, 8), np.float32), hits=np.zeros((4, 4), np.float32),
                              out=np.zeros((4, 24), np.float32))),                                    # out= with host inputs
        (ctx.shade_hits, dict(rays=np.zeros((4, 8), np.float64), hits=np.zeros((4, 4), np.float32))),  # host dtype
        (ctx.shade_hits, dict(rays=np.zeros((4, 8), np.float32), hits=np.zeros((5, 4), np.float32))),  # host lengths
        (ctx.sample_bsdf, dict(surfaces=surf, seeds=FakeGpuTensor((64,), torch.float32))),            # seed dtype
        (ctx.sample_bsdf, dict(surfaces=surf, seeds=FakeGpuTensor((64, 1), torch.int32))),            # seed rank
        (ctx.sample_bsdf, dict(surfaces=FakeGpuTensor((64, 20), torch.float32), seeds=seeds)),        # record width
        (ctx.sample_bsdf, dict(surfaces=surf, seeds=seeds, mat_index=2)),                             # material model
        (ctx.sample_bsdf, dict(surfaces=surf, seeds=seeds, out=FakeGpuTensor((64, 4), torch.float32))),  # out shape
        (ctx.eval_bsdf, dict(surfaces=surf, dirs=FakeGpuTensor((64, 3), torch.float32))),             # dirs shape
        (ctx.eval_bsdf, dict(surfaces=surf, dirs=FakeGpuTensor((64, 4), torch.int32))),               # dirs dtype
        (ctx.eval_bsdf, dict(surfaces=surf, dirs=dirs, mat_index=-1)),                                # material model
        (ctx.eval_bsdf, dict(surfaces=surf, dirs=dirs, out=FakeGpuTensor((64, 4), torch.int32))),     # out dtype
        (ctx.camera_rays, dict(gparams=gp, width=0, height=9)),                                       # empty frame
        (ctx.camera_rays, dict(gparams=gp, width=65536, height=65536)),                               # 2^32 rays
        (ctx.camera_rays, dict(gparams=object(), width=16, height=9)),                                # not GBufferParams
        (ctx.camera_rays, dict(gparams=gp, width=16, height=9, out=FakeGpuTensor((143, 8), torch.float32))),  # out shape
        (ctx.camera_rays, dict(gparams=gp, width=16, height=9, out=FakeGpuTensor((144, 8), torch.float16))),  # out dtype
    ]
    for fn, kw in bad:
        with pytest.raises(pkg.BdptError):
            fn(**kw)
    assert ctx._lib.calls == []


def test_host_inputs_never_reach_the_library_as_device_pointers(pkg, monkeypatch):
    """numpy arrays and CPU tensors are copied to the device and only the copies' addresses reach the library; without a
    GPU the call is refused before the library is reached."""
    import torch
    ctx = _context_without_device(pkg)
    rays, hits = torch.zeros(5, 8), np.zeros((5, 4), np.int32)
    if not torch.cuda.is_available():
        with pytest.raises(pkg.BdptError):
            ctx.shade_hits(rays, hits)
        assert ctx._lib.calls == []
    copies = []

    def fake_copy(a, dev):
        assert isinstance(a, np.ndarray)
        copies.append(FakeGpuTensor(a.shape, {np.float32: torch.float32, np.int32: torch.int32,
                                              np.uint32: torch.uint32}[a.dtype.type], ptr=0x20000 + 0x1000 * len(copies)))
        return copies[-1]

    monkeypatch.setattr(pkg, "_host_to_device", fake_copy)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "device", lambda d: _NullContext())
    monkeypatch.setattr(torch, "empty", lambda shape, dtype, device: _FakeOut(shape, dtype))
    ctx.shade_hits(rays, hits)
    call = ctx._lib.calls[-1]
    assert (call["rays"], call["hits"]) == (copies[0].data_ptr(), copies[1].data_ptr())
    assert call["rays"] != rays.data_ptr() and call["hits"] != hits.ctypes.data and call["out"] == 0x90000
    ctx.sample_bsdf(np.zeros((5, 24), np.float32), np.arange(5, dtype=np.uint32))
    call = ctx._lib.calls[-1]
    assert (call["surfaces"], call["seeds"]) == (copies[2].data_ptr(), copies[3].data_ptr())


# ---- numpy float32 restatements (the GPU tests compare the device against them bit for bit) ----
F = np.float32


def _normalize(v):
    inv = F(1.0) / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    return v * inv[:, None]


def pinhole_rays(cam, width, height, jitter):
    """primaryRay's pinhole branch (device_scene.hpp) in its operation order: (N, 8) bdpt_ray records."""
    U, V, W, P = (np.array(getattr(cam, n)[:], F) for n in ("cameraU", "cameraV", "cameraW", "posW"))
    y, x = np.divmod(np.arange(width * height, dtype=np.int64), width)
    pcx = (x.astype(F) + F(jitter[0])) / F(width)
    pcy = (y.astype(F) + F(jitter[1])) / F(height)
    ndx = F(2.0) * pcx + F(-1.0)
    ndy = F(-2.0) * pcy + F(1.0)
    d = (U[None] * ndx[:, None] + V[None] * ndy[:, None]) + W[None]
    d = d / np.sqrt((W[0] * W[0] + W[1] * W[1]) + W[2] * W[2])
    d = _normalize(d)
    n = width * height
    return np.concatenate([np.broadcast_to(P, (n, 3)), np.zeros((n, 1), F), d, np.full((n, 1), 1e38, F)], axis=1).astype(F)


def shade_geometry(desc, origins, prim, bu, bv):
    """shadeHit's position, unmapped normal, V and dist (+ the double-sided flip) for hits with prim >= 0, in its
    operation order: posW (N, 3), N (N, 3), V (N, 3), dist (N,)."""
    idx = np.ctypeslib.as_array(desc.indices, shape=(desc.numTriangles, 3))[prim]
    pos = np.ctypeslib.as_array(desc.positions, shape=(desc.numVertices, 3))
    nrm = np.ctypeslib.as_array(desc.normals, shape=(desc.numVertices, 3))
    bu, bv = bu.astype(F)[:, None], bv.astype(F)[:, None]
    b0 = (F(1.0) - bu) - bv
    posW = ((np.zeros_like(bu) + pos[idx[:, 0]] * b0) + pos[idx[:, 1]] * bu) + pos[idx[:, 2]] * bv
    nW = ((np.zeros_like(bu) + nrm[idx[:, 0]] * b0) + nrm[idx[:, 1]] * bu) + nrm[idx[:, 2]] * bv
    N = _normalize(_normalize(nW))
    V = _normalize(origins - posW)
    dv = posW - origins
    dist = np.sqrt((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2])
    mats = np.ctypeslib.as_array(desc.triMaterial, shape=(desc.numTriangles,))[prim]
    flags = np.array([desc.materials[int(m)].flags for m in range(desc.numMaterials)], np.uint32)[mats]
    ndv = (N[:, 0] * V[:, 0] + N[:, 1] * V[:, 1]) + N[:, 2] * V[:, 2]
    flip = (ndv <= 0) & (((flags >> 19) & 1) != 0)
    N = np.where(flip[:, None], -N, N)
    return posW.astype(F), N.astype(F), V.astype(F), dist.astype(F)


def test_numpy_restatement_matches_the_oracle_gbuffer(pkg, ob):
    """The restatements above against the CPU oracle: pinhole rays traced by oracle_trace (back faces culled) and shaded
    give oracle_gbuffer's WorldPosition bit for bit and its WorldNormal (N, dist) after half rounding, on a scene without
    normal maps."""
    W, H = 48, 32
    scene = pkg.Scene.cornell()
    cam = scene.camera(W / H)
    gp = pkg.abi.GBufferParams()
    gp.pixelJitter[0], gp.pixelJitter[1] = pkg.msaa_jitter(0xdeadbeef)
    gp.frameCount, gp.focalLen, gp.lensRadius = 0xdeadbeef, 1.0, 1.0 / 64.0
    gp.envColor[:] = [0.5, 0.5, 0.8, 1.0]
    orc = ob.OracleRender(pkg.abi, scene.desc, W, H)
    orc.gbuffer(cam, gp)
    rays = pinhole_rays(cam, W, H, gp.pixelJitter)
    lib = ob.load_oracle(pkg.abi)
    o_rays = np.ascontiguousarray(np.concatenate([rays[:, 0:3], rays[:, 4:7], rays[:, 3:4], rays[:, 7:8]], axis=1))
    prim = np.zeros(W * H, np.int32)
    tuv = np.zeros((W * H, 3), np.float32)
    lib.oracle_trace(orc.scene, o_rays.ctypes.data, W * H, 1, 0, prim.ctypes.data, tuv.ctypes.data)
    hit = prim >= 0
    assert 0 < hit.sum() < W * H
    pos = orc.chan["worldPosition"]
    assert np.array_equal(pos[:, 3] != 0, hit)
    posW, N, V, dist = shade_geometry(scene.desc, rays[hit, 0:3], prim[hit], tuv[hit, 1], tuv[hit, 2])
    assert np.array_equal(pos[hit, :3].view(np.uint32), posW.view(np.uint32))
    half = np.zeros((int(hit.sum()), 4), np.float32)
    nd = np.ascontiguousarray(np.concatenate([N, dist[:, None]], axis=1), np.float32)
    lib.oracle_half_round(nd.ctypes.data, nd.size, half.ctypes.data)
    assert np.array_equal(orc.chan["worldNormal"][hit].view(np.uint32), half.view(np.uint32))
    orc.close()
    scene.close()
