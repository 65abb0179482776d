"""CPU checks of bdpt_execute_grouped's interface (include/bdpt.h "Assignable light groups"): declared in the header,
exported by the library and bound in abi.py; the descriptor's layout against the header's declaration; the argument errors
that need no device; and the Python layer's refusals, raised before any device is touched."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AREA = 4096


def _header():
    return open(os.path.join(ROOT, "include", "bdpt.h")).read()


def test_grouped_declared_exported_and_bound(pkg):
    hdr = _header()
    assert re.search(r"int bdpt_execute_grouped\(bdpt_ctx\* ctx, const bdpt_params\* p, const bdpt_gbuffer\* in, float\* out, "
                     r"const bdpt_light_group_desc\* desc,\s*void\* stream\);", hdr)
    m = re.search(r"#define BDPT_PREPARE_LIGHT_GROUP_TABLE (\d+)u", hdr)
    a = pkg.abi
    assert m and int(m.group(1)) == a.PREPARE_LIGHT_GROUP_TABLE == 32
    others = a.PREPARE_PRIMARY | a.PREPARE_BMFR | a.PREPARE_REFIT | a.PREPARE_LIGHT_GROUPS | a.PREPARE_AREA_LIGHTS
    assert a.PREPARE_LIGHT_GROUP_TABLE & others == 0
    so = os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "csrc", "libbdpt_amd.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT bdpt_execute_grouped$", syms, flags=re.M)
    res, args = a.PROTOTYPES["bdpt_execute_grouped"]
    assert res is C.c_int and len(args) == 6 and args[4] == C.POINTER(a.LightGroupDesc)
    lib = pkg.load_library()
    assert lib.bdpt_execute_grouped.argtypes == args


# (size, alignment) of the C types the descriptor uses, LP64
_CTYPES = {"float*": (8, 8), "const uint8_t*": (8, 8), "uint32_t": (4, 4)}


def test_descriptor_layout_matches_the_header(pkg):
    """Offsets and size worked out from the header's own declaration by the C layout rules."""
    m = re.search(r"typedef struct bdpt_light_group_desc \{(.*?)\} bdpt_light_group_desc;", _header(), flags=re.S)
    assert m
    fields = []
    for line in m.group(1).splitlines():
        line = re.sub(r"/\*.*?\*/", "", line).strip()
        if not line:
            continue
        d = re.match(r"(.+?)\s*(\w+)(?:\[(\d+)\])?;$", line)
        assert d, line
        fields.append((d.group(2), d.group(1).strip(), int(d.group(3) or 1)))
    assert [f[0] for f in fields] == ["planes", "numGroups", "numAssigned", "groupOf", "reserved"]
    off, align_max, want = 0, 1, {}
    for name, ctype, count in fields:
        size, align = _CTYPES[ctype]
        off = (off + align - 1) // align * align
        want[name] = off
        off += size * count
        align_max = max(align_max, align)
    total = (off + align_max - 1) // align_max * align_max
    d = pkg.abi.LightGroupDesc
    assert [n for n, _ in d._fields_] == [f[0] for f in fields]
    assert {n: getattr(d, n).offset for n, _ in d._fields_} == want
    assert C.sizeof(d) == total == 32
    assert d.reserved.size == 8 and d.groupOf.size == 8


def test_grouped_null_arguments(pkg):
    """NULL context, descriptor, planes or groupOf: BDPT_E_INVALID, before anything looks for a device."""
    lib = pkg.load_library()
    a = pkg.abi
    p, g, d = a.Params(), a.GBuffer(), a.LightGroupDesc()
    one = (C.c_uint8 * 1)(0)
    d.planes, d.numGroups, d.numAssigned, d.groupOf = 16, 1, 1, C.cast(one, C.POINTER(C.c_uint8))
    assert lib.bdpt_execute_grouped(None, C.byref(p), C.byref(g), C.c_void_p(16), C.byref(d), None) == -1
    assert lib.bdpt_execute_grouped(None, C.byref(p), C.byref(g), C.c_void_p(16), None, None) == -1
    assert lib.bdpt_execute_grouped(None, None, None, None, None, None) == -1
    d.planes = None
    assert lib.bdpt_execute_grouped(None, C.byref(p), C.byref(g), C.c_void_p(16), C.byref(d), None) == -1
    d.planes, d.groupOf = 16, None
    assert lib.bdpt_execute_grouped(None, C.byref(p), C.byref(g), C.c_void_p(16), C.byref(d), None) == -1
    # (the same on a real context: tests/test_gpu_light_group_assign.py)


class _Desc:
    numLights = 3


class _Scene:
    desc = _Desc()


@pytest.mark.parametrize("groups, flags, what", [
    ([0, 1], 0, "3 entries"), ([0, 1, 0, 1], 0, "3 entries"), ([0, 1, 0], AREA, "4 entries"), ([], 0, "3 entries"),
    ([0, 17, 0], 0, "0 .. 16"), ([0, 1, 0, 17], AREA, "0 .. 16"), ([0, -1, 0], 0, "0 .. 16")])
def test_pipeline_refuses_a_bad_assignment(pkg, groups, flags, what):
    with pytest.raises(pkg.BdptError, match=what):
        pkg.FramePipeline(_Scene(), 64, 64, light_groups=groups, flags=flags)


@pytest.mark.parametrize("kw", [dict(stripes=(8, 2, 0)), dict(stripes=(4, 1, 0)), dict(tile=(0, 32)), dict(tile=(16, 64))])
def test_pipeline_refuses_a_list_on_part_of_the_frame(pkg, kw):
    with pytest.raises(pkg.BdptError, match="whole frame"):
        pkg.FramePipeline(_Scene(), 64, 64, light_groups=[0, 1, 0], **kw)


def test_context_binding_fills_the_descriptor(pkg):
    """Context.execute_grouped hands the library a descriptor with the planes, the counts and a copy of the assignment."""
    calls = []

    class Lib:
        def bdpt_execute_grouped(self, h, p, g, out, d, stream):
            d = d._obj
            calls.append((h.value, p._obj.maxDepth, out.value, d.planes, d.numGroups, d.numAssigned,
                          [d.groupOf[i] for i in range(d.numAssigned)], list(d.reserved), stream))
            return self.rc

        def bdpt_last_error(self, h):
            return b"execute_grouped: reserved must be 0"

    ctx = pkg.Context.__new__(pkg.Context)
    ctx._lib, ctx._h, ctx.device = Lib(), C.c_void_p(7), 0
    Lib.rc = 0
    p = pkg.abi.Params()
    p.maxDepth = 5
    g = pkg.abi.GBuffer()
    ctx.execute_grouped(p, g, C.c_void_p(0x1000), C.c_void_p(0x2000), (0, 2, 1, 2), 3, "stream")
    assert calls == [(7, 5, 0x1000, 0x2000, 3, 4, [0, 2, 1, 2], [0, 0], "stream")]
    Lib.rc = -1
    with pytest.raises(pkg.BdptError, match="reserved must be 0"):
        ctx.execute_grouped(p, g, C.c_void_p(0x1000), C.c_void_p(0x2000), [0], 1)
    with pytest.raises(pkg.BdptError, match="0 .. 255"):
        ctx.execute_grouped(p, g, C.c_void_p(0x1000), C.c_void_p(0x2000), [300], 1)
    ctx._h = None
