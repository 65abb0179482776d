"""CPU checks of bdpt_bmfr_execute_planes (include/bdpt.h "Denoised planes"): the ctypes structure against the header, the
symbols, the error codes that need no GPU, and the binding's own argument checks and what it hands to the library.  The
kernels are tested on the GPU by tests/test_gpu_bmfr_planes.py."""
import ctypes as C

import pytest

from binding_fakes import FakeGpuTensor, RecordingLib, context_without_device, desc_fields, header_layout

FIELDS = ["planes", "numPlanes", "reserved", "prevPosition"]
SYMBOLS = ["bdpt_bmfr_execute_planes", "bdpt_bmfr_planes_prepare", "bdpt_bmfr_planes_reset"]
H, W = 6, 10


def test_planes_struct_and_symbols_match_the_header(pkg):
    a, lib = pkg.abi, pkg.load_library()
    lay = header_layout({"bdpt_bmfr_planes_desc": FIELDS}, {"consts": ["BDPT_BMFR_MAX_PLANES", "BDPT_MAX_LIGHTS"]})
    assert int(lay["bdpt_bmfr_planes_desc"]) == C.sizeof(a.BmfrPlanesDesc) == 24
    assert [n for n, _ in a.BmfrPlanesDesc._fields_] == FIELDS
    for f in FIELDS:
        assert int(lay[f"bdpt_bmfr_planes_desc.{f}"]) == getattr(a.BmfrPlanesDesc, f).offset, f
    assert lay["consts"] == f"{a.BMFR_MAX_PLANES} {a.BDPT_MAX_LIGHTS}" == "18 16"
    for n in SYMBOLS:
        assert hasattr(lib, n) and n in a.PROTOTYPES, n
    for n in ("bmfr_execute_planes", "bmfr_planes_prepare", "bmfr_planes_reset"):
        assert callable(getattr(pkg.Context, n)), n
    assert callable(pkg.FramePipeline.denoise_reset) and callable(pkg.view_proj_of_camera)


def test_planes_null_arguments(pkg):
    """BDPT_E_INVALID for a NULL context, params, features or desc before anything touches a device"""
    a, lib = pkg.abi, pkg.load_library()
    bp, gb, d = a.BmfrParams(), a.GBuffer(), a.BmfrPlanesDesc()
    assert lib.bdpt_bmfr_execute_planes(None, C.byref(bp), C.byref(gb), C.byref(d), None) == -1
    assert lib.bdpt_bmfr_planes_prepare(None, 1) == -1
    assert lib.bdpt_bmfr_planes_reset(None) == -1


def _lib():
    def record(params, gbuffer, desc, stream):
        f = desc_fields(desc)
        f["planes"] = [desc.planes[k] for k in range(desc.numPlanes)]  # (read while the binding's array is alive)
        return ("execute_planes", params.frameNumber, f, stream)
    return RecordingLib({"bdpt_bmfr_execute_planes": record,
                         "bdpt_bmfr_planes_prepare": lambda n: ("prepare", n),
                         "bdpt_bmfr_planes_reset": lambda: ("reset",)})


def _tensor(shape, torch, **kw):
    return FakeGpuTensor(shape, torch.float32, **kw)


def test_binding_hands_the_library_one_pointer_per_plane(pkg):
    import torch
    a = pkg.abi
    lib = _lib()
    ctx = context_without_device(pkg, lib)
    p, gb = a.BmfrParams(), a.GBuffer()
    p.frameNumber = 7
    ctx.bmfr_planes_prepare(3)
    ctx.bmfr_planes_reset()
    ctx.bmfr_execute_planes(p, gb, _tensor((3, H, W, 4), torch, ptr=0x4000), None, 55)
    ctx.bmfr_execute_planes(p, gb, [_tensor((H, W, 4), torch, ptr=0x9000), _tensor((H, W, 4), torch, ptr=0x1000)],
                            _tensor((H, W, 4), torch, ptr=0x7000))
    assert lib.calls[0] == ("prepare", 3) and lib.calls[1] == ("reset",)
    step = H * W * 16
    assert lib.calls[2] == ("execute_planes", 7, {"planes": [0x4000, 0x4000 + step, 0x4000 + 2 * step], "numPlanes": 3,
                                                  "reserved": 0, "prevPosition": None}, 55)
    assert lib.calls[3] == ("execute_planes", 7, {"planes": [0x9000, 0x1000], "numPlanes": 2, "reserved": 0,
                                                  "prevPosition": 0x7000}, None)


def test_binding_refuses_before_the_library_is_called(pkg):
    import torch
    a = pkg.abi
    lib = _lib()
    ctx = context_without_device(pkg, lib)
    ctx._frame = (H, W)  # (what resize records)
    p, gb = a.BmfrParams(), a.GBuffer()
    ok = _tensor((2, H, W, 4), torch)
    one = _tensor((H, W, 4), torch)
    cases = [
        (FakeGpuTensor((2, H, W, 4), torch.float64), None, "float32"),
        (_tensor((2, H, W, 4), torch, contiguous=False), None, "contiguous"),
        (_tensor((2, H, W, 4), torch, index=1), None, "cuda:0"),
        (_tensor((2, H, W, 3), torch), None, r"\(P, H, W, 4\)"),
        (_tensor((H, W, 4), torch), None, r"\(P, H, W, 4\)"),
        (_tensor((2, H + 1, W, 4), torch), None, "whole frames"),
        (_tensor((0, H, W, 4), torch), None, "1 .. 18 planes"),
        (_tensor((a.BMFR_MAX_PLANES + 1, H, W, 4), torch), None, "1 .. 18 planes"),
        ([], None, "1 .. 18 planes"),
        ([one] * (a.BMFR_MAX_PLANES + 1), None, "1 .. 18 planes"),
        ([one, _tensor((H, W + 1, 4), torch)], None, r"planes\[1\]"),
        ([one, FakeGpuTensor((H, W, 4), torch.float16)], None, r"planes\[1\]"),
        ([one, torch.zeros(H, W, 4)], None, "GPU tensor"),
        ([_tensor((H, W), torch)], None, r"planes\[0\]"),
        (7, None, "sequence"),
        (ok, _tensor((H, W, 3), torch), "prev_position"),
        (ok, FakeGpuTensor((H, W, 4), torch.float16), "prev_position"),
        (ok, torch.zeros(H, W, 4), "prev_position"),
    ]
    for planes, prev, match in cases:
        with pytest.raises(pkg.BdptError, match=match):
            ctx.bmfr_execute_planes(p, gb, planes, prev)
    assert lib.calls == []
    ctx.bmfr_execute_planes(p, gb, ok)
    assert len(lib.calls) == 1
