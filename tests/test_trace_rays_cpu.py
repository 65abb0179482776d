"""CPU checks of bdpt_trace_rays' interface: the ctypes structures against include/bdpt.h, and the Python binding's
argument checks (Context.trace_rays) against a fake library, so that nothing a GPU would need is involved."""
import ctypes as C

import numpy as np
import pytest

from binding_fakes import FakeGpuTensor, RecordingLib, _FakeOut, _NullContext, context_without_device, header_layout

STRUCTS = {
    "bdpt_ray": ["org", "tmin", "dir", "tmax"],
    "bdpt_hit": ["t", "u", "v", "prim"],
    "bdpt_trace_desc": ["rays", "numRays", "mode", "numRaysDevice", "hits", "visible"],
}


def test_trace_structs_match_the_header(pkg):
    a = pkg.abi
    lay = header_layout(STRUCTS, {"modes": ["BDPT_TRACE_CLOSEST", "BDPT_TRACE_CLOSEST_CULL_BACK", "BDPT_TRACE_ANY"]},
                        lang="c++")
    assert int(lay["bdpt_ray"]) == C.sizeof(a.Ray) == 32
    assert int(lay["bdpt_hit"]) == C.sizeof(a.Hit) == 16
    assert int(lay["bdpt_trace_desc"]) == C.sizeof(a.TraceDesc)
    for cls, cname in ((a.Ray, "bdpt_ray"), (a.Hit, "bdpt_hit"), (a.TraceDesc, "bdpt_trace_desc")):
        for name, _ in cls._fields_:
            assert int(lay[f"{cname}.{name}"]) == getattr(cls, name).offset, (cname, name)
    assert lay["modes"] == f"{a.TRACE_CLOSEST} {a.TRACE_CLOSEST_CULL_BACK} {a.TRACE_ANY}"
    assert "bdpt_trace_rays" in a.PROTOTYPES


def _context_without_device(pkg, device=0):
    """a Context whose library records what bdpt_trace_rays is handed"""
    return context_without_device(pkg, RecordingLib({"bdpt_trace_rays": lambda d, stream: dict(
        rays=d.rays, numRays=d.numRays, mode=d.mode, count=d.numRaysDevice, hits=d.hits, visible=d.visible)}), device)


def test_host_rays_never_reach_the_library_as_device_pointers(pkg, monkeypatch):
    """numpy arrays and CPU tensors take the host path: a device copy is made and only its address reaches
    bdpt_trace_rays.  Without a GPU the call is refused before the library is reached."""
    import torch
    ctx = _context_without_device(pkg)
    rays = torch.zeros(5, 8)
    arr = np.zeros((5, 8), np.float32)
    if not torch.cuda.is_available():
        for r in (rays, arr):
            with pytest.raises(pkg.BdptError):
                ctx.trace_rays(r)
        assert ctx._lib.calls == []
    # with the device copy stubbed (and no synchronise to do), what reaches the library is the copy's address
    copies = []

    def fake_copy(a, dev):
        assert isinstance(a, np.ndarray) and a.shape == (5, 8) and a.dtype == np.float32
        copies.append(FakeGpuTensor(a.shape, torch.float32, ptr=0x20000 + 0x1000 * len(copies)))
        return copies[-1]

    monkeypatch.setattr(pkg, "_host_to_device", fake_copy)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "device", lambda d: _NullContext())
    monkeypatch.setattr(torch, "empty", lambda shape, dtype, device: _FakeOut(shape, dtype))
    for r in (rays, arr):
        ctx.trace_rays(r, mode="any")
        call = ctx._lib.calls[-1]
        assert call["rays"] == copies[-1].data_ptr()
        assert call["rays"] not in (rays.data_ptr(), arr.ctypes.data)
        assert call["numRays"] == 5 and call["mode"] == pkg.abi.TRACE_ANY and call["visible"] is not None
    assert len(ctx._lib.calls) == 2


def test_bad_arguments_are_refused_before_the_library(pkg):
    import torch
    ctx = _context_without_device(pkg)
    good = FakeGpuTensor((64, 8), torch.float32)
    tuv, prim = ctx.trace_rays(good, out=FakeGpuTensor((64, 4), torch.float32, ptr=0x30000))
    assert ctx._lib.calls[-1]["rays"] == 0x10000 and ctx._lib.calls[-1]["hits"] == 0x30000
    ctx.trace_rays(good, mode="any", out=FakeGpuTensor((64,), torch.uint8, ptr=0x40000),
                   count=FakeGpuTensor((1,), torch.int32, ptr=0x50000))
    assert ctx._lib.calls[-1]["visible"] == 0x40000 and ctx._lib.calls[-1]["count"] == 0x50000
    ctx.trace_rays(good, mode="closest_cull_back", out=FakeGpuTensor((64, 4), torch.int32, ptr=0x30000),
                   count=FakeGpuTensor((1,), torch.uint32, ptr=0x50000))
    assert ctx._lib.calls[-1]["mode"] == pkg.abi.TRACE_CLOSEST_CULL_BACK
    for shape in ((), (1, 1)):  # any one-element count, not only (1,)
        ctx.trace_rays(good, out=FakeGpuTensor((64, 4), torch.float32), count=FakeGpuTensor(shape, torch.int32, ptr=0x50000))
        assert ctx._lib.calls[-1]["count"] == 0x50000
    calls = len(ctx._lib.calls)
    bad = [
        dict(rays=FakeGpuTensor((64, 8), torch.float32, index=1)),                         # another GPU
        dict(rays=FakeGpuTensor((64, 8), torch.float64)),                                  # dtype
        dict(rays=FakeGpuTensor((64, 7), torch.float32)),                                  # shape
        dict(rays=FakeGpuTensor((64, 2, 4), torch.float32)),                               # rank
        dict(rays=FakeGpuTensor((64, 8), torch.float32, contiguous=False)),                # strides
        dict(rays=good, mode="nearest"),                                                   # mode
        dict(rays=good, out=FakeGpuTensor((64, 4), torch.float32, index=1)),               # out on another GPU
        dict(rays=good, out=FakeGpuTensor((64, 3), torch.float32)),                        # out shape
        dict(rays=good, out=FakeGpuTensor((64, 4), torch.float16)),                        # out dtype
        dict(rays=good, out=FakeGpuTensor((64, 4), torch.float32, contiguous=False)),      # out strides
        dict(rays=good, mode="any", out=FakeGpuTensor((64,), torch.int32)),                # visibility dtype
        dict(rays=good, mode="any", out=FakeGpuTensor((63,), torch.uint8)),                # visibility length
        dict(rays=good, count=FakeGpuTensor((1,), torch.int64)),                           # count dtype
        dict(rays=good, count=FakeGpuTensor((2,), torch.int32)),                           # count size
        dict(rays=good, count=FakeGpuTensor((1,), torch.int32, index=1)),                  # count device
        dict(rays=good, count=torch.ones(1, dtype=torch.int32)),                           # count in host memory
        dict(rays=np.zeros((4, 8), np.float32), out=np.zeros((4, 4), np.float32)),        # out= with host rays
        dict(rays=np.zeros((4, 8), np.float64)),                                           # host dtype
        dict(rays=torch.zeros(4, 6)),                                                      # host shape
    ]
    for kw in bad:
        with pytest.raises(pkg.BdptError):
            ctx.trace_rays(**kw)
    assert len(ctx._lib.calls) == calls
