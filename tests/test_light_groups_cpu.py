"""CPU checks of bdpt_execute_light_groups' interface: declared in include/bdpt.h, exported by the library, bound in
abi.py; the argument errors that need no device; and the Python layer's refusal of a pipeline that does not render the
whole frame (refused before any device is touched)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_light_groups_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "bdpt.h")).read()
    assert re.search(r"int bdpt_execute_light_groups\(bdpt_ctx\* ctx, const bdpt_params\* p, const bdpt_gbuffer\* in, "
                     r"float\* out, float\* groups, void\* stream\);", hdr)
    m = re.search(r"#define BDPT_PREPARE_LIGHT_GROUPS (\d+)u", hdr)
    assert m and int(m.group(1)) == pkg.abi.PREPARE_LIGHT_GROUPS
    # (distinct from the other prepare bits)
    assert pkg.abi.PREPARE_LIGHT_GROUPS & (pkg.abi.PREPARE_PRIMARY | pkg.abi.PREPARE_BMFR | pkg.abi.PREPARE_REFIT) == 0
    so = os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "csrc", "libbdpt_amd.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT bdpt_execute_light_groups$", syms, flags=re.M)
    res, args = pkg.abi.PROTOTYPES["bdpt_execute_light_groups"]
    assert res is C.c_int and len(args) == 6
    lib = pkg.load_library()
    assert lib.bdpt_execute_light_groups.argtypes == args


def test_light_groups_null_arguments(pkg):
    """A NULL context, with or without groups, is BDPT_E_INVALID — before anything looks for a device."""
    lib = pkg.load_library()
    a = pkg.abi
    p = a.Params()
    g = a.GBuffer()
    assert lib.bdpt_execute_light_groups(None, C.byref(p), C.byref(g), None, None, None) == -1
    assert lib.bdpt_execute_light_groups(None, C.byref(p), C.byref(g), C.c_void_p(16), C.c_void_p(16), None) == -1
    assert lib.bdpt_execute_light_groups(None, None, None, None, None, None) == -1


class _Desc:
    numLights = 3


class _Scene:
    desc = _Desc()


@pytest.mark.parametrize("kw", [dict(stripes=(8, 2, 0)), dict(stripes=(4, 1, 0)), dict(tile=(0, 32)), dict(tile=(16, 64))])
def test_pipeline_refuses_light_groups_on_part_of_the_frame(pkg, kw):
    with pytest.raises(pkg.BdptError, match="whole frame"):
        pkg.FramePipeline(_Scene(), 64, 64, light_groups=True, **kw)


def test_context_binding_passes_both_pointers(pkg):
    """Context.execute_light_groups hands the library the params, channels, out, groups and stream it is given."""
    calls = []

    class Lib:
        def bdpt_execute_light_groups(self, h, p, g, out, groups, stream):
            calls.append((h.value, p._obj.maxDepth, g._obj.emissive, out.value, groups.value, stream))
            return 0

        def bdpt_last_error(self, h):
            return b""

    ctx = pkg.Context.__new__(pkg.Context)
    ctx._lib, ctx._h, ctx.device = Lib(), C.c_void_p(7), 0
    p = pkg.abi.Params()
    p.maxDepth = 5
    g = pkg.abi.GBuffer()
    g.emissive = 0x3000
    ctx.execute_light_groups(p, g, C.c_void_p(0x1000), C.c_void_p(0x2000), "stream")
    assert calls == [(7, 5, 0x3000, 0x1000, 0x2000, "stream")]

    class Failing(Lib):
        def bdpt_execute_light_groups(self, *a):
            return -1

        def bdpt_last_error(self, h):
            return b"light groups: groups is NULL"

    ctx._lib = Failing()
    with pytest.raises(pkg.BdptError, match="groups is NULL"):
        ctx.execute_light_groups(p, g, C.c_void_p(0x1000), None)
    ctx._h = None
