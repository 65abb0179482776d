"""CPU checks of MIS sky lighting (bdpt_bsdf_pdf_query, bdpt_sky_mis_query, bdpt_sky_mis_execute): the ctypes structures
against include/bdpt.h, declaration / export / binding of the entry points, the Python binding's argument passing and checks
against a fake library, FramePipeline.sky_lighting's defaults and its MIS switch, and bdpt_render's new options."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import env_numpy as en
from binding_fakes import ROOT, FakeGpuTensor, RecordingLib, context_without_device, desc_fields, header_layout

F, U = np.float32, np.uint32
STRUCTS = {
    "bdpt_bsdf_pdf_desc": ("BsdfPdfDesc", ["num", "matIndex", "numDevice", "flags", "reserved", "surfaces", "dirs", "values"]),
    "bdpt_sky_mis_desc": ("SkyMisDesc", ["num", "samples", "numDevice", "clampUpper", "minT", "matIndex", "techniques", "flags", "reserved",
                                          "surfaces", "seeds", "alive", "color", "counts", "seedsOut"]),
    "bdpt_sky_mis_params": ("SkyMisParams", ["frameCount", "clampUpper", "minT", "samples", "matIndex", "techniques", "reserved"]),
    # the plain pass's structures stay byte for byte
    "bdpt_sky_desc": ("SkyDesc", ["num", "samples", "numDevice", "clampUpper", "minT", "flags", "reserved", "surfaces", "seeds", "alive", "color",
                                  "counts", "seedsOut"]),
    "bdpt_sky_params": ("SkyParams", ["frameCount", "clampUpper", "minT", "samples", "reserved"]),
}
ENTRY_POINTS = ["bdpt_bsdf_pdf_query", "bdpt_sky_mis_query", "bdpt_sky_mis_execute"]


def test_structs_match_the_header(pkg):
    a = pkg.abi
    lay = header_layout({c: f for c, (_, f) in STRUCTS.items()}, {"C": ["BDPT_SKY_MIS_TABLE", "BDPT_SKY_MIS_BSDF", "BDPT_SKY_MAX_SAMPLES"]})
    for cname, (pyname, fields) in STRUCTS.items():
        cls = getattr(a, pyname)
        assert int(lay[cname]) == C.sizeof(cls), cname
        assert [n for n, _ in cls._fields_] == fields, cname
        for name in fields:
            assert int(lay[f"{cname}.{name}"]) == getattr(cls, name).offset, (cname, name)
    assert [C.sizeof(getattr(a, n)) for n in ("BsdfPdfDesc", "SkyMisDesc", "SkyMisParams", "SkyDesc", "SkyParams")] == [48, 88, 32, 80, 20]
    assert [int(v) for v in lay["C"].split()] == [a.SKY_MIS_TABLE, a.SKY_MIS_BSDF, a.SKY_MAX_SAMPLES] == [1, 2, 64]
    # the library asserts the same sizes where it fills the device structures
    src = open(os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "csrc", "api_query.cpp")).read()
    assert re.search(r"static_assert\(sizeof\(bdpt_bsdf_pdf_desc\) == 48 .*sizeof\(bdpt_sky_mis_desc\) == 88 .*\n.*sizeof\(bdpt_sky_mis_params\) == 32", src)


def test_the_entry_points_are_declared_exported_and_bound(pkg):
    a = pkg.abi
    src = open(os.path.join(ROOT, "include", "bdpt.h")).read()
    assert re.search(r"int\s+bdpt_bsdf_pdf_query\(bdpt_ctx\*\s*\w+,\s*const bdpt_bsdf_pdf_desc\*\s*\w+,\s*void\*\s*\w+\);", src)
    assert re.search(r"int\s+bdpt_sky_mis_query\(bdpt_ctx\*\s*\w+,\s*const bdpt_sky_mis_desc\*\s*\w+,\s*void\*\s*\w+\);", src)
    assert re.search(r"int\s+bdpt_sky_mis_execute\(bdpt_ctx\*\s*\w+,\s*const bdpt_sky_mis_params\*\s*\w+,\s*const bdpt_gbuffer\*\s*\w+,"
                     r"\s*float\*\s*\w+,\s*void\*\s*\w+\);", src)
    section = src[src.index("/* MIS sky lighting"):src.index("#define BDPT_SKY_MIS_TABLE")]
    for text in ("probabilityToSampleDiffuse", "exactly three draws", "L_0, B_0, L_1, B_1", "balance heuristic", "bit for bit", "e.pdf + pB",
                 "ev.pdf + pB", "2 * samples", "record contract"):
        assert text in section, text
    assert a.PROTOTYPES["bdpt_bsdf_pdf_query"] == (C.c_int, [C.c_void_p, C.POINTER(a.BsdfPdfDesc), C.c_void_p])
    assert a.PROTOTYPES["bdpt_sky_mis_query"] == (C.c_int, [C.c_void_p, C.POINTER(a.SkyMisDesc), C.c_void_p])
    assert a.PROTOTYPES["bdpt_sky_mis_execute"] == (C.c_int, [C.c_void_p, C.POINTER(a.SkyMisParams), C.POINTER(a.GBuffer), C.c_void_p,
                                                              C.c_void_p])
    raw = C.CDLL(a.LIB_PATH)
    lib = pkg.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(raw, name) and name in a.PROTOTYPES, name
        assert getattr(lib, name).argtypes == a.PROTOTYPES[name][1]
    assert lib.bdpt_bsdf_pdf_query(None, None, None) == -1 and lib.bdpt_sky_mis_query(None, None, None) == -1  # BDPT_E_INVALID
    assert lib.bdpt_sky_mis_execute(None, None, None, None, None) == -1
    # the new kernel is its own file in the library's build; the plain pass's file is not touched by it
    mk = open(os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "csrc", "Makefile")).read()
    assert " sky.o " in mk and " sky_mis.o " in mk and "device_bsdf_pdf.hpp" in mk


def _ctx(pkg, device=0):
    return context_without_device(pkg, RecordingLib({
        "bdpt_bsdf_pdf_query": lambda d, stream: desc_fields(d), "bdpt_sky_mis_query": lambda d, stream: desc_fields(d),
        "bdpt_sky_mis_execute": lambda p, gb, out, stream: ("mis", desc_fields(p), gb, out, stream),
        "bdpt_sky_execute": lambda p, gb, out, stream: ("plain", desc_fields(p), gb, out, stream),
        "bdpt_env_prepare": lambda stream: ("prepare", stream), "bdpt_set_environment": lambda e: ("set", desc_fields(e))}), device)


def test_good_calls_reach_the_library(pkg):
    import torch
    a = pkg.abi
    ctx = _ctx(pkg)
    f32, i32, u32, u8 = torch.float32, torch.int32, torch.uint32, torch.uint8
    n = 70
    surf, seeds = FakeGpuTensor((n, 24), f32, ptr=0x10000), FakeGpuTensor((n,), u32, ptr=0x20000)
    dirs, val, cnt = FakeGpuTensor((n, 4), f32, ptr=0x11000), FakeGpuTensor((n, 4), f32, ptr=0x12000), FakeGpuTensor((1,), i32, ptr=0x50000)
    assert ctx.bsdf_pdf(surf, dirs, 1, out=val, count=cnt) is val
    assert ctx._lib.calls[-1] == dict(num=n, matIndex=1, numDevice=0x50000, flags=0, reserved=0, surfaces=0x10000, dirs=0x11000, values=0x12000)
    ctx.bsdf_pdf(surf, dirs, out=val)
    assert (ctx._lib.calls[-1]["matIndex"], ctx._lib.calls[-1]["numDevice"]) == (0, None)  # GGX by default, as sample_bsdf
    col, alive, counts = FakeGpuTensor((n, 4), f32, ptr=0x13000), FakeGpuTensor((n,), u8, ptr=0x14000), FakeGpuTensor((n,), u32, ptr=0x15000)
    assert ctx.sky_lighting_mis(surf, seeds, 7, mat_index=1, techniques=2, clamp=2.5, min_t=0.5, alive=alive, out=col, counts=counts,
                                seeds_out=seeds, count=cnt) is col
    assert ctx._lib.calls[-1] == dict(num=n, samples=7, numDevice=0x50000, clampUpper=2.5, minT=0.5, matIndex=1, techniques=2, flags=0,
                                      reserved=0, surfaces=0x10000, seeds=0x20000, alive=0x14000, color=0x13000, counts=0x15000,
                                      seedsOut=0x20000)
    ctx.sky_lighting_mis(surf, seeds, 64, out=col)
    c = ctx._lib.calls[-1]
    assert (c["clampUpper"], c["samples"], c["matIndex"], c["techniques"], c["minT"], c["alive"]) == (en.FLT_MAX, 64, 0, 3, F(1e-4), None)
    p, gb = a.SkyMisParams(3, 1.0, 1e-4, 8, 0, 3), a.GBuffer()
    ctx.sky_mis_execute(p, gb, 0x1234, "stream")
    kind, fields, gb_seen, out_seen, st = ctx._lib.calls[-1]
    assert kind == "mis" and gb_seen is gb and (out_seen, st) == (0x1234, "stream")
    assert fields == dict(frameCount=3, clampUpper=1.0, minT=F(1e-4), samples=8, matIndex=0, techniques=3, reserved=[0, 0])


def test_bad_arguments_are_refused_before_the_library(pkg):
    import torch
    ctx = _ctx(pkg)
    f32, i32, u32, u8 = torch.float32, torch.int32, torch.uint32, torch.uint8
    n = 64
    surf, seeds, dirs = FakeGpuTensor((n, 24), f32), FakeGpuTensor((n,), u32), FakeGpuTensor((n, 4), f32)
    good = dict(surfaces=surf, seeds=seeds, samples=4)
    bad_sky = [
        dict(good, samples=0), dict(good, samples=65), dict(good, samples=2.0), dict(good, samples=True), dict(good, samples=None),
        dict(good, mat_index=2), dict(good, mat_index=True), dict(good, mat_index=-1), dict(good, techniques=0), dict(good, techniques=4),
        dict(good, techniques=True), dict(good, techniques=1.0), dict(good, techniques=None),
        dict(good, surfaces=FakeGpuTensor((n, 24), f32, index=1)), dict(good, surfaces=FakeGpuTensor((n, 20), f32)),
        dict(good, surfaces=FakeGpuTensor((n, 24), f32, contiguous=False)), dict(good, seeds=FakeGpuTensor((n,), f32)),
        dict(good, seeds=FakeGpuTensor((n - 1,), u32)), dict(good, seeds=np.zeros(n, U)), dict(good, alive=FakeGpuTensor((n,), torch.bool)),
        dict(good, alive=FakeGpuTensor((n + 1,), u8)), dict(good, out=FakeGpuTensor((n,), f32)), dict(good, out=FakeGpuTensor((n, 4), i32)),
        dict(good, out=torch.zeros(n, 4)), dict(good, counts=FakeGpuTensor((n,), f32)), dict(good, seeds_out=FakeGpuTensor((n, 1), u32)),
        dict(good, count=FakeGpuTensor((2,), u32)), dict(good, count=torch.ones(1, dtype=i32)),
        dict(surfaces=np.zeros((n, 24), F), seeds=np.zeros(n, U), samples=4, counts=FakeGpuTensor((n,), u32)),
    ]
    for kw in bad_sky:
        with pytest.raises(pkg.BdptError):
            ctx.sky_lighting_mis(**kw)
    good = dict(surfaces=surf, dirs=dirs)
    bad_pdf = [
        dict(good, mat_index=2), dict(good, mat_index=True), dict(good, surfaces=FakeGpuTensor((n, 23), f32)), dict(good, dirs=FakeGpuTensor((n, 3), f32)),
        dict(good, dirs=FakeGpuTensor((n, 4), torch.float64)), dict(good, dirs=FakeGpuTensor((n, 4), f32, index=1)),
        dict(good, dirs=FakeGpuTensor((n + 1, 4), f32)), dict(good, dirs=np.zeros((n, 4), F)), dict(good, out=FakeGpuTensor((n, 8), f32)),
        dict(good, out=FakeGpuTensor((n, 4), i32)), dict(good, count=FakeGpuTensor((2,), u32)),
    ]
    for kw in bad_pdf:
        with pytest.raises(pkg.BdptError):
            ctx.bsdf_pdf(**kw)
    assert ctx._lib.calls == []


def _pipe(pkg, ctx):
    import torch
    pipe = pkg.FramePipeline.__new__(pkg.FramePipeline)
    pipe.ctx, pipe.min_t, pipe.gb, pipe.sky_frame, pipe.last_sky_params = ctx, 0.5, pkg.abi.GBuffer(), 0, None
    pipe.torch, pipe.dev, pipe.H, pipe.W = torch, None, 2, 3
    pipe.channels = {pkg.SKY_CHANNEL: FakeGpuTensor((2, 3, 4), torch.float32, ptr=0x5000)}
    pipe._stream_ptr = lambda: "stream"
    return pipe


def test_frame_pipeline_sky_lighting_defaults_and_its_mis_switch(pkg):
    """the defaults make exactly the plain pass's call; mis=True hands Context.sky_mis_execute the same frame counter, min_t,
    G-buffer and stream with both techniques on; the counter is shared; GGX without MIS is refused"""
    a = pkg.abi
    ctx = _ctx(pkg)
    pipe = _pipe(pkg, ctx)
    ctx.set_environment(0x9000, 8, 4)
    out = pipe.sky_lighting(samples=8, clamp=2.0)
    assert out is pipe.channels[pkg.SKY_CHANNEL] and ctx._lib.calls[-2] == ("prepare", "stream")
    kind, fields, gb, ptr, st = ctx._lib.calls[-1]
    assert kind == "plain" and fields == dict(frameCount=0, clampUpper=2.0, minT=0.5, samples=8, reserved=0)
    assert gb is pipe.gb and st == "stream" and ptr.value == 0x5000 and isinstance(pipe.last_sky_params, a.SkyParams)
    pipe.sky_lighting()
    assert ctx._lib.calls[-1][:2] == ("plain", dict(frameCount=1, clampUpper=en.FLT_MAX, minT=0.5, samples=1, reserved=0))
    n = len(ctx._lib.calls)
    out = pipe.sky_lighting(4, 3.0, mis=True)
    assert out is pipe.channels[pkg.SKY_CHANNEL] and len(ctx._lib.calls) == n + 1  # the table is the same one
    kind, fields, gb, ptr, st = ctx._lib.calls[-1]
    assert kind == "mis" and fields == dict(frameCount=2, clampUpper=3.0, minT=0.5, samples=4, matIndex=1, techniques=3, reserved=[0, 0])
    assert gb is pipe.gb and st == "stream" and ptr.value == 0x5000 and isinstance(pipe.last_sky_params, a.SkyMisParams)
    pipe.sky_lighting(2, mis=True, mat_index=0)
    assert ctx._lib.calls[-1][1] == dict(frameCount=3, clampUpper=en.FLT_MAX, minT=0.5, samples=2, matIndex=0, techniques=3, reserved=[0, 0])
    ctx.set_environment(0xA000, 8, 4)  # a new probe: prepared anew on the MIS path too
    pipe.sky_lighting(2, mis=True)
    assert ctx._lib.calls[-2] == ("prepare", "stream") and ctx._lib.calls[-1][1]["frameCount"] == 4
    n = len(ctx._lib.calls)
    for kw in (dict(mat_index=0), dict(mis=True, mat_index=2), dict(mis=True, mat_index=True), dict(mis=True, samples=0), dict(mis=True, samples=65)):
        with pytest.raises(pkg.BdptError):
            pipe.sky_lighting(**kw)
    assert len(ctx._lib.calls) == n and pipe.sky_frame == 5


def test_bdpt_render_new_options():
    """--sky-mis without --sky N and --sky-ggx without --sky-mis exit 2 with a message before any GPU is touched; the usage
    text names both"""
    render = os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "host", "bdpt_render")
    if not os.path.exists(render):
        pytest.skip("host/bdpt_render not built")
    for args in (["--sky-mis"], ["--sky-mis", "--sky-ggx"], ["--env", "probe.hdr", "--sky", "4", "--sky-ggx"]):
        r = subprocess.run([render] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--sky-mis goes with --sky N" in r.stderr, (args, r.stderr)
    u = subprocess.run([render, "--help"], capture_output=True, text=True, timeout=60)
    assert "[--sky N [--sky-clamp C] [--sky-mis [--sky-ggx]]]" in u.stderr


def test_sky_pass_has_the_mis_switches():
    """SkyLightingPass::setMis / setMaterial under the reference-style names; the checkpoint record is the plain pass's"""
    import shutil
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    host = os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "host")
    src = ('#include "ReferenceNames.h"\nint main() {\n  SkyLightingPass::SharedPtr sky = SkyLightingPass::create();\n  sky->setMis(true);\n'
           "  sky->setMaterial(0);\n  sky->setClamp(2.0f);\n  return sky ? 0 : 1;\n}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + host, "-x", "c++", "-"],
                       input=src, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
