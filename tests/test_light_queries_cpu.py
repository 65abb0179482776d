"""CPU checks of the light queries' interface (bdpt_light_query): the ctypes structures and constants against
include/bdpt.h, and the Python binding's argument checks against a fake library, so that nothing a GPU would need is
involved."""
import ctypes as C

import numpy as np
import pytest

from binding_fakes import (FakeGpuTensor, RecordingLib, _FakeOut, _NullContext, context_without_device, desc_fields,
                           header_layout)

STRUCTS = {
    "bdpt_light_sample": ("LightSample", ["ray", "value", "light", "status"]),
    "bdpt_light_emit": ("LightEmit", ["ray", "color", "light"]),
    "bdpt_light_desc": ("LightDesc", ["mode", "num", "numDevice", "matIndex", "flags", "minT", "reserved", "surfaces", "seeds",
                                      "seedsOut", "samples", "emits", "compactRays", "compactItems", "compactCount"]),
}
CONSTS = ["BDPT_LIGHT_NEE", "BDPT_LIGHT_EMIT", "BDPT_LIGHT_USE_HINTS", "BDPT_LIGHT_STATUS_NONZERO", "BDPT_LIGHT_STATUS_HINT_OCCLUDED",
          "BDPT_PARAM_AREA_LIGHTS"]


def test_light_structs_match_the_header(pkg):
    a = pkg.abi
    lay = header_layout({c: f for c, (_, f) in STRUCTS.items()}, {c: [c] for c in CONSTS})
    assert int(lay["bdpt_light_sample"]) == C.sizeof(a.LightSample) == 48  # three float4
    assert int(lay["bdpt_light_emit"]) == C.sizeof(a.LightEmit) == 48
    for cname, (pyname, fields) in STRUCTS.items():
        cls = getattr(a, pyname)
        assert int(lay[cname]) == C.sizeof(cls), cname
        assert [n for n, _ in cls._fields_] == fields, cname
        for name in fields:
            assert int(lay[f"{cname}.{name}"]) == getattr(cls, name).offset, (cname, name)
    # light and status share the record's last word: light | status << 16 when read as one uint32
    assert (a.LightSample.light.offset, a.LightSample.status.offset) == (44, 46)
    got = [int(lay[c]) for c in CONSTS]
    assert got == [a.LIGHT_NEE, a.LIGHT_EMIT, a.LIGHT_USE_HINTS, a.LIGHT_STATUS_NONZERO, a.LIGHT_STATUS_HINT_OCCLUDED,
                   a.PARAM_AREA_LIGHTS]
    assert a.LIGHT_USE_HINTS & a.PARAM_AREA_LIGHTS == 0  # the two share the flags word


def test_the_prototype_is_declared(pkg):
    a = pkg.abi
    assert a.PROTOTYPES["bdpt_light_query"] == (C.c_int, [C.c_void_p, C.POINTER(a.LightDesc), C.c_void_p])


def _context_without_device(pkg, device=0):
    """a Context whose library records what bdpt_light_query is handed"""
    return context_without_device(pkg, RecordingLib({"bdpt_light_query": lambda d, stream: desc_fields(d)}), device)


def test_good_calls_reach_the_library(pkg):
    import torch
    a = pkg.abi
    ctx = _context_without_device(pkg)
    surf = FakeGpuTensor((64, 24), torch.float32, ptr=0x10000)
    seeds = FakeGpuTensor((64,), torch.uint32, ptr=0x20000)
    out = FakeGpuTensor((64, 12), torch.float32, ptr=0x30000)
    cnt = FakeGpuTensor((1,), torch.uint32, ptr=0x40000)
    so = FakeGpuTensor((64,), torch.int32, ptr=0x50000)
    comp = (FakeGpuTensor((64, 8), torch.float32, ptr=0x60000), FakeGpuTensor((64,), torch.int32, ptr=0x70000),
            FakeGpuTensor((1,), torch.int32, ptr=0x80000))
    ctx.sample_lights(surf, seeds, mat_index=1, min_t=0.25, area_lights=True, use_hints=True, out=out, seeds_out=so, compact=comp,
                      count=cnt)
    c = ctx._lib.calls[-1]
    assert c == dict(mode=a.LIGHT_NEE, num=64, numDevice=0x40000, matIndex=1, flags=a.PARAM_AREA_LIGHTS | a.LIGHT_USE_HINTS, minT=0.25,
                     reserved=0, surfaces=0x10000, seeds=0x20000, seedsOut=0x50000, samples=0x30000, emits=None, compactRays=0x60000,
                     compactItems=0x70000, compactCount=0x80000)
    ctx.sample_lights(FakeGpuTensor((64, 24), torch.int32, ptr=0x10000), FakeGpuTensor((64,), torch.int32, ptr=0x20000),
                      out=FakeGpuTensor((64, 12), torch.int32, ptr=0x30000))
    c = ctx._lib.calls[-1]
    assert (c["flags"], c["matIndex"], c["numDevice"], c["seedsOut"], c["compactRays"], c["compactItems"], c["compactCount"]) == (
        0, 0, None, None, None, None, None)
    assert c["minT"] == np.float32(1e-4)
    ctx.emit_lights(seeds, min_t=0.5, area_lights=True, out=out, seeds_out=so, count=cnt)
    c = ctx._lib.calls[-1]
    assert c == dict(mode=a.LIGHT_EMIT, num=64, numDevice=0x40000, matIndex=0, flags=a.PARAM_AREA_LIGHTS, minT=0.5, reserved=0,
                     surfaces=None, seeds=0x20000, seedsOut=0x50000, samples=None, emits=0x30000, compactRays=None, compactItems=None,
                     compactCount=None)
    ctx.emit_lights(seeds, out=out)
    assert ctx._lib.calls[-1]["flags"] == 0 and ctx._lib.calls[-1]["seedsOut"] is None


def test_bad_arguments_are_refused_before_the_library(pkg):
    import torch
    ctx = _context_without_device(pkg)
    f32, i32, u32 = torch.float32, torch.int32, torch.uint32
    surf, seeds = FakeGpuTensor((64, 24), f32), FakeGpuTensor((64,), i32)
    rays, items, cc = FakeGpuTensor((64, 8), f32), FakeGpuTensor((64,), u32), FakeGpuTensor((1,), u32)
    nee, emit = ctx.sample_lights, ctx.emit_lights
    bad = [
        (nee, dict(surfaces=FakeGpuTensor((64, 24), torch.float64), seeds=seeds)),              # surfaces dtype
        (nee, dict(surfaces=FakeGpuTensor((64, 20), f32), seeds=seeds)),                        # record width
        (nee, dict(surfaces=FakeGpuTensor((64, 24), f32, index=1), seeds=seeds)),               # another GPU
        (nee, dict(surfaces=FakeGpuTensor((64, 24), f32, contiguous=False), seeds=seeds)),      # strides
        (nee, dict(surfaces=surf, seeds=FakeGpuTensor((64,), f32))),                            # seed dtype
        (nee, dict(surfaces=surf, seeds=FakeGpuTensor((64, 1), i32))),                          # seed rank
        (nee, dict(surfaces=surf, seeds=FakeGpuTensor((63,), i32))),                            # lengths differ
        (nee, dict(surfaces=surf, seeds=torch.zeros(64, dtype=i32))),                           # GPU and CPU tensors mixed
        (nee, dict(surfaces=torch.zeros(64, 24), seeds=seeds)),                                 # the other way round
        (nee, dict(surfaces=surf, seeds=seeds, mat_index=2)),                                   # material model
        (nee, dict(surfaces=surf, seeds=seeds, out=FakeGpuTensor((64, 8), f32))),               # out shape
        (nee, dict(surfaces=surf, seeds=seeds, out=FakeGpuTensor((64, 12), torch.float16))),    # out dtype
        (nee, dict(surfaces=surf, seeds=seeds, seeds_out=FakeGpuTensor((64,), f32))),           # seeds_out dtype
        (nee, dict(surfaces=surf, seeds=seeds, seeds_out=FakeGpuTensor((32,), i32))),           # seeds_out length
        (nee, dict(surfaces=surf, seeds=seeds, seeds_out=torch.zeros(64, dtype=i32))),          # seeds_out on the host
        (nee, dict(surfaces=surf, seeds=seeds, count=FakeGpuTensor((1,), torch.int64))),        # count dtype
        (nee, dict(surfaces=surf, seeds=seeds, count=FakeGpuTensor((2,), i32))),                # count size
        (nee, dict(surfaces=surf, seeds=seeds, count=torch.ones(1, dtype=i32))),                # count on the host
        (nee, dict(surfaces=surf, seeds=seeds, compact=(rays, items, None))),                   # compaction in part
        (nee, dict(surfaces=surf, seeds=seeds, compact=(rays, None, cc))),
        (nee, dict(surfaces=surf, seeds=seeds, compact=(None, items, cc))),
        (nee, dict(surfaces=surf, seeds=seeds, compact=(rays, items))),
        (nee, dict(surfaces=surf, seeds=seeds, compact=rays)),
        (nee, dict(surfaces=surf, seeds=seeds, compact=(FakeGpuTensor((64, 7), f32), items, cc))),   # compact rays shape
        (nee, dict(surfaces=surf, seeds=seeds, compact=(FakeGpuTensor((32, 8), f32), items, cc))),   # capacity below N
        (nee, dict(surfaces=surf, seeds=seeds, compact=(rays, FakeGpuTensor((64,), f32), cc))),      # items dtype
        (nee, dict(surfaces=surf, seeds=seeds, compact=(rays, items, FakeGpuTensor((2,), u32)))),    # count size
        (nee, dict(surfaces=surf, seeds=seeds, compact=(rays, items, torch.zeros(1, dtype=i32)))),   # count on the host
        (nee, dict(surfaces=np.zeros((4, 24), np.float32), seeds=np.zeros(4, np.uint32),
                   out=np.zeros((4, 12), np.float32))),                                         # out= with host inputs
        (nee, dict(surfaces=np.zeros((4, 24), np.float32), seeds=np.zeros(4, np.uint32),
                   seeds_out=FakeGpuTensor((4,), i32))),                                        # seeds_out= with host inputs
        (nee, dict(surfaces=np.zeros((4, 24), np.float32), seeds=np.zeros(4, np.uint32),
                   compact=(FakeGpuTensor((4, 8), f32), FakeGpuTensor((4,), i32), cc))),        # compact= with host inputs
        (nee, dict(surfaces=np.zeros((4, 24), np.float64), seeds=np.zeros(4, np.uint32))),      # host dtype
        (nee, dict(surfaces=np.zeros((4, 24), np.float32), seeds=np.zeros(5, np.uint32))),      # host lengths
        (nee, dict(surfaces=np.zeros((4, 24), np.float32), seeds=np.zeros(4, np.float32))),     # host seed dtype
        (emit, dict(seeds=FakeGpuTensor((64,), f32))),                                          # seed dtype
        (emit, dict(seeds=FakeGpuTensor((64, 1), i32))),                                        # seed rank
        (emit, dict(seeds=FakeGpuTensor((64,), i32, index=1))),                                 # another GPU
        (emit, dict(seeds=seeds, out=FakeGpuTensor((64, 8), f32))),                             # out shape
        (emit, dict(seeds=seeds, seeds_out=FakeGpuTensor((64, 1), i32))),                       # seeds_out rank
        (emit, dict(seeds=seeds, count=FakeGpuTensor((1,), f32))),                              # count dtype
        (emit, dict(seeds=np.zeros((4, 1), np.uint32))),                                        # host seed rank
        (emit, dict(seeds=np.zeros(4, np.uint32), count=cc)),                                   # count= with host inputs
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
    surf, seeds = torch.zeros(5, 24), np.arange(5, dtype=np.uint32)
    if not torch.cuda.is_available():
        with pytest.raises(pkg.BdptError):
            ctx.sample_lights(surf, seeds)
        with pytest.raises(pkg.BdptError):
            ctx.emit_lights(seeds)
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
    ctx.sample_lights(surf, seeds, mat_index=1)
    call = ctx._lib.calls[-1]
    assert (call["surfaces"], call["seeds"]) == (copies[0].data_ptr(), copies[1].data_ptr())
    assert call["surfaces"] != surf.data_ptr() and call["seeds"] != seeds.ctypes.data and call["samples"] == 0x90000
    ctx.emit_lights(seeds)
    call = ctx._lib.calls[-1]
    assert call["seeds"] == copies[2].data_ptr() and call["emits"] == 0x90000 and call["mode"] == pkg.abi.LIGHT_EMIT
