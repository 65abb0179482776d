"""CPU checks of the connection queries' interface (bdpt_connect_query, bdpt_splat_add): the ctypes structures and
constants against include/bdpt.h, and the Python binding's argument checks against a fake library, so that nothing a GPU
would need is involved."""
import ctypes as C

import numpy as np
import pytest

from binding_fakes import FakeGpuTensor, RecordingLib, context_without_device, desc_fields, header_layout

STRUCTS = {
    "bdpt_connect_sample": ("ConnectSample", ["ray", "value", "status"]),
    "bdpt_camera_sample": ("CameraSample", ["ray", "f", "G", "pixel", "status", "reserved"]),
    "bdpt_connect_desc": ("ConnectDesc", ["mode", "num", "numDevice", "matIndex", "flags", "minT", "reserved", "eye", "light", "eyePrev",
                                          "lightPrev", "eyeSpecular", "lightSpecular", "samples", "cameraSamples", "width", "height",
                                          "pixelJitter", "compactRays", "compactItems", "compactCount"]),
    "bdpt_splat_desc": ("SplatDesc", ["num", "numPixels", "numDevice", "pixels", "values", "visible", "items", "splat"]),
}
CONSTS = ["BDPT_CONNECT_VERTICES", "BDPT_CONNECT_CAMERA", "BDPT_CONNECT_STATUS_NONZERO", "BDPT_CONNECT_STATUS_PIXEL"]


def test_connect_structs_match_the_header(pkg):
    a = pkg.abi
    lay = header_layout({c: f for c, (_, f) in STRUCTS.items()}, {c: [c] for c in CONSTS})
    assert int(lay["bdpt_connect_sample"]) == C.sizeof(a.ConnectSample) == 48  # three float4
    assert int(lay["bdpt_camera_sample"]) == C.sizeof(a.CameraSample) == 64    # four float4
    for cname, (pyname, fields) in STRUCTS.items():
        cls = getattr(a, pyname)
        assert int(lay[cname]) == C.sizeof(cls), cname
        assert [n for n, _ in cls._fields_] == fields, cname
        for name in fields:
            assert int(lay[f"{cname}.{name}"]) == getattr(cls, name).offset, (cname, name)
    # the columns the bindings document: value 8-10, status 11; f 8-10, G 11, pixel 12, status 13
    assert (a.ConnectSample.value.offset, a.ConnectSample.status.offset) == (32, 44)
    assert (a.CameraSample.f.offset, a.CameraSample.G.offset, a.CameraSample.pixel.offset, a.CameraSample.status.offset) == (32, 44, 48, 52)
    got = [int(lay[c]) for c in CONSTS]
    assert got == [a.CONNECT_VERTICES, a.CONNECT_CAMERA, a.CONNECT_STATUS_NONZERO, a.CONNECT_STATUS_PIXEL] == [0, 1, 1, 2]


def test_the_prototypes_are_declared(pkg):
    a = pkg.abi
    assert a.PROTOTYPES["bdpt_connect_query"] == (C.c_int, [C.c_void_p, C.POINTER(a.ConnectDesc), C.c_void_p])
    assert a.PROTOTYPES["bdpt_splat_add"] == (C.c_int, [C.c_void_p, C.POINTER(a.SplatDesc), C.c_void_p])


def _context_without_device(pkg, device=0):
    """a Context whose library records what the two entry points are handed"""
    record = lambda d, stream: desc_fields(d)  # noqa: E731
    return context_without_device(pkg, RecordingLib({"bdpt_connect_query": record, "bdpt_splat_add": record}), device)


def test_good_calls_reach_the_library(pkg):
    import torch
    a = pkg.abi
    ctx = _context_without_device(pkg)
    f32, i32, u32, u8 = torch.float32, torch.int32, torch.uint32, torch.uint8
    eye, light = FakeGpuTensor((64, 24), f32, ptr=0x10000), FakeGpuTensor((64, 24), i32, ptr=0x20000)
    ep, lp = FakeGpuTensor((64, 4), f32, ptr=0x30000), FakeGpuTensor((64, 4), f32, ptr=0x40000)
    es, ls = FakeGpuTensor((64,), u8, ptr=0x50000), FakeGpuTensor((64,), u8, ptr=0x60000)
    out = FakeGpuTensor((64, 12), f32, ptr=0x70000)
    cnt = FakeGpuTensor((1,), u32, ptr=0x80000)
    comp = (FakeGpuTensor((64, 8), f32, ptr=0x90000), FakeGpuTensor((64,), i32, ptr=0xa0000), FakeGpuTensor((1,), i32, ptr=0xb0000))
    ctx.connect_vertices(eye, light, mat_index=1, min_t=0.25, eye_prev=ep, light_prev=lp, eye_specular=es, light_specular=ls, out=out,
                         compact=comp, count=cnt)
    assert ctx._lib.calls[-1] == dict(
        mode=a.CONNECT_VERTICES, num=64, numDevice=0x80000, matIndex=1, flags=0, minT=0.25, reserved=0, eye=0x10000, light=0x20000,
        eyePrev=0x30000, lightPrev=0x40000, eyeSpecular=0x50000, lightSpecular=0x60000, samples=0x70000, cameraSamples=None, width=0,
        height=0, pixelJitter=[0.0, 0.0], compactRays=0x90000, compactItems=0xa0000, compactCount=0xb0000)
    ctx.connect_vertices(eye, light, out=out)
    c = ctx._lib.calls[-1]
    assert [c[k] for k in ("eyePrev", "lightPrev", "eyeSpecular", "lightSpecular", "numDevice", "compactRays", "compactItems",
                           "compactCount")] == [None] * 8
    assert c["matIndex"] == 0 and c["minT"] == np.float32(1e-4)
    cam = FakeGpuTensor((64, 16), i32, ptr=0xc0000)
    ctx.connect_camera(light, 72, 56, pixel_jitter=(0.25, 0.75), mat_index=0, min_t=0.5, light_specular=ls, out=cam, compact=comp,
                       count=cnt)
    assert ctx._lib.calls[-1] == dict(
        mode=a.CONNECT_CAMERA, num=64, numDevice=0x80000, matIndex=0, flags=0, minT=0.5, reserved=0, eye=None, light=0x20000,
        eyePrev=None, lightPrev=None, eyeSpecular=None, lightSpecular=0x60000, samples=None, cameraSamples=0xc0000, width=72, height=56,
        pixelJitter=[0.25, 0.75], compactRays=0x90000, compactItems=0xa0000, compactCount=0xb0000)
    splat = FakeGpuTensor((4032, 4), torch.int64, ptr=0xd0000)
    pixels, values = FakeGpuTensor((64,), i32, ptr=0xe0000), FakeGpuTensor((64, 4), f32, ptr=0xf0000)
    items, vis = FakeGpuTensor((40,), u32, ptr=0x100000), FakeGpuTensor((40,), u8, ptr=0x110000)
    ctx.splat_add(splat, pixels, values, visible=vis, items=items, count=cnt)
    assert ctx._lib.calls[-1] == dict(num=40, numPixels=4032, numDevice=0x80000, pixels=0xe0000, values=0xf0000, visible=0x110000,
                                      items=0x100000, splat=0xd0000)
    ctx.splat_add(splat, pixels, values)
    c = ctx._lib.calls[-1]
    assert (c["num"], c["visible"], c["items"], c["numDevice"]) == (64, None, None, None)
    ctx.splat_add((0x120000, 4 * 4032), pixels, values)  # what Context.splat_buffer() returns: the context's own buffer
    c = ctx._lib.calls[-1]
    assert (c["splat"], c["numPixels"], c["num"]) == (0x120000, 4032, 64)


def test_bad_arguments_are_refused_before_the_library(pkg):
    import torch
    ctx = _context_without_device(pkg)
    f32, i32, u32, u8 = torch.float32, torch.int32, torch.uint32, torch.uint8
    surf, other = FakeGpuTensor((64, 24), f32), FakeGpuTensor((64, 24), f32)
    rays, items, cc = FakeGpuTensor((64, 8), f32), FakeGpuTensor((64,), u32), FakeGpuTensor((1,), u32)
    splat, pixels, values = FakeGpuTensor((100, 4), torch.int64), FakeGpuTensor((64,), u32), FakeGpuTensor((64, 4), f32)
    ver, cam, add = ctx.connect_vertices, ctx.connect_camera, ctx.splat_add
    camkw = dict(light=surf, width=8, height=8)
    addkw = dict(splat=splat, pixels=pixels, values=values)
    bad = [
        (ver, dict(eye=np.zeros((4, 24), np.float32), light=np.zeros((4, 24), np.float32))),     # host arrays
        (ver, dict(eye=torch.zeros(4, 24), light=torch.zeros(4, 24))),                           # CPU tensors
        (ver, dict(eye=surf, light=torch.zeros(64, 24))),                                        # GPU and CPU mixed
        (ver, dict(eye=FakeGpuTensor((64, 24), torch.float64), light=other)),                    # dtype
        (ver, dict(eye=FakeGpuTensor((64, 20), f32), light=other)),                              # record width
        (ver, dict(eye=surf, light=FakeGpuTensor((63, 24), f32))),                               # lengths differ
        (ver, dict(eye=surf, light=FakeGpuTensor((64, 24), f32, index=1))),                      # another GPU
        (ver, dict(eye=FakeGpuTensor((64, 24), f32, contiguous=False), light=other)),            # strides
        (ver, dict(eye=surf, light=other, mat_index=2)),                                         # material model
        (ver, dict(eye=surf, light=other, eye_prev=FakeGpuTensor((64, 3), f32))),                # predecessor width
        (ver, dict(eye=surf, light=other, light_prev=FakeGpuTensor((32, 4), f32))),              # predecessor length
        (ver, dict(eye=surf, light=other, light_prev=torch.zeros(64, 4))),                       # predecessor on the host
        (ver, dict(eye=surf, light=other, eye_specular=FakeGpuTensor((64,), i32))),              # specular bytes dtype
        (ver, dict(eye=surf, light=other, light_specular=FakeGpuTensor((64, 1), u8))),           # specular bytes rank
        (ver, dict(eye=surf, light=other, out=FakeGpuTensor((64, 16), f32))),                    # out shape
        (ver, dict(eye=surf, light=other, out=FakeGpuTensor((64, 12), torch.float16))),          # out dtype
        (ver, dict(eye=surf, light=other, count=FakeGpuTensor((1,), torch.int64))),              # count dtype
        (ver, dict(eye=surf, light=other, count=torch.ones(1, dtype=i32))),                      # count on the host
        (ver, dict(eye=surf, light=other, compact=(rays, items, None))),                         # compaction in part
        (ver, dict(eye=surf, light=other, compact=(rays, None, cc))),
        (ver, dict(eye=surf, light=other, compact=(None, items, cc))),
        (ver, dict(eye=surf, light=other, compact=(rays, items))),
        (ver, dict(eye=surf, light=other, compact=rays)),
        (ver, dict(eye=surf, light=other, compact=(FakeGpuTensor((32, 8), f32), items, cc))),    # capacity below N
        (ver, dict(eye=surf, light=other, compact=(rays, FakeGpuTensor((64,), f32), cc))),       # items dtype
        (ver, dict(eye=surf, light=other, compact=(rays, items, torch.zeros(1, dtype=i32)))),    # count on the host
        (cam, dict(light=np.zeros((4, 24), np.float32), width=8, height=8)),                     # host array
        (cam, dict(light=surf, width=0, height=8)),                                              # frame size
        (cam, dict(light=surf, width=8, height=0)),
        (cam, dict(light=surf, width=65536, height=65536)),
        (cam, dict(camkw, pixel_jitter=(0.5,))),                                                 # jitter
        (cam, dict(camkw, mat_index=True)),                                                      # material model
        (cam, dict(camkw, out=FakeGpuTensor((64, 12), f32))),                                    # out shape
        (cam, dict(camkw, light_specular=FakeGpuTensor((63,), u8))),                             # specular bytes length
        (cam, dict(camkw, compact=(rays, items, None))),                                         # compaction in part
        (cam, dict(camkw, compact=(None, None, cc))),
        (cam, dict(camkw, compact=(FakeGpuTensor((64, 7), f32), items, cc))),                    # compact rays shape
        (add, dict(addkw, splat=np.zeros((100, 4), np.int64))),                                  # host arrays
        (add, dict(addkw, pixels=np.zeros(64, np.uint32))),
        (add, dict(addkw, values=torch.zeros(64, 4))),
        (add, dict(addkw, splat=None)),                                                          # required
        (add, dict(addkw, splat=(0x1000, 4030))),                                                # not whole pixels
        (add, dict(addkw, splat=(0, 4032))),                                                     # a NULL buffer
        (add, dict(addkw, splat=(0x1000, 4032, 1))),
        (add, dict(addkw, splat=FakeGpuTensor((100, 3), torch.int64))),                          # words per pixel
        (add, dict(addkw, splat=FakeGpuTensor((100, 4), f32))),                                  # splat dtype
        (add, dict(addkw, splat=FakeGpuTensor((400,), torch.int64))),                            # splat rank
        (add, dict(addkw, pixels=FakeGpuTensor((64,), f32))),                                    # pixels dtype
        (add, dict(addkw, pixels=FakeGpuTensor((64, 1), u32))),                                  # pixels rank
        (add, dict(addkw, values=FakeGpuTensor((64, 3), f32))),                                  # values width
        (add, dict(addkw, values=FakeGpuTensor((63, 4), f32))),                                  # values length
        (add, dict(addkw, visible=FakeGpuTensor((63,), u8))),                                    # one byte per entry
        (add, dict(addkw, visible=FakeGpuTensor((64,), i32))),                                   # visible dtype
        (add, dict(addkw, items=FakeGpuTensor((40,), f32))),                                     # items dtype
        (add, dict(addkw, items=FakeGpuTensor((40,), u32), visible=FakeGpuTensor((64,), u8))),   # visible goes by entry
        (add, dict(addkw, items=torch.zeros(40, dtype=i32))),                                    # items on the host
        (add, dict(addkw, count=FakeGpuTensor((2,), u32))),                                      # count size
        (add, dict(addkw, splat=FakeGpuTensor((100, 4), torch.int64, index=1))),                 # another GPU
    ]
    for fn, kw in bad:
        with pytest.raises(pkg.BdptError):
            fn(**kw)
    assert ctx._lib.calls == []
