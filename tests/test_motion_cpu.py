"""CPU checks of the motion interface (include/bdpt.h "Motion": bdpt_keep_pose, bdpt_gbuffer_execute_motion,
bdpt_motion_query, bdpt_bmfr_execute_motion): the library's symbols, the ctypes structure against the header, the error
codes that need no GPU, and the C++ host's channel and switch.  The kernels are tested on the GPU by tests/test_motion.py."""
import ctypes as C
import os
import subprocess
import tempfile

from binding_fakes import header_layout

FIELDS = ["hits", "num", "reserved", "numDevice", "prevPositions"]
SYMBOLS = ["bdpt_keep_pose", "bdpt_gbuffer_execute_motion", "bdpt_motion_query", "bdpt_bmfr_execute_motion"]


def test_motion_symbols_and_struct_match_the_header(pkg):
    a, lib = pkg.abi, pkg.load_library()
    lay = header_layout({"bdpt_motion_desc": FIELDS, "bdpt_bmfr_params": []}, {"consts": ["BDPT_PREPARE_MOTION"]})
    assert int(lay["bdpt_motion_desc"]) == C.sizeof(a.MotionDesc) == 32
    assert [n for n, _ in a.MotionDesc._fields_] == FIELDS
    for f in FIELDS:
        assert int(lay[f"bdpt_motion_desc.{f}"]) == getattr(a.MotionDesc, f).offset, f
    assert int(lay["bdpt_bmfr_params"]) == C.sizeof(a.BmfrParams) == 72  # (ABI: the motion call takes the same params)
    assert lay["consts"] == str(a.PREPARE_MOTION) == "64"
    for n in SYMBOLS:
        assert hasattr(lib, n) and n in a.PROTOTYPES, n
    for n in ("keep_pose", "motion_query", "gbuffer_execute_motion", "bmfr_execute_motion"):
        assert callable(getattr(pkg.Context, n)), n
    assert callable(pkg.FramePipeline.motion_query)


def test_motion_null_arguments(pkg):
    """BDPT_E_INVALID for a NULL context (or params / channels / desc) before anything touches a device"""
    a, lib = pkg.abi, pkg.load_library()
    gp, gb, bp, d = a.GBufferParams(), a.GBuffer(), a.BmfrParams(), a.MotionDesc()
    assert lib.bdpt_keep_pose(None, None) == -1
    assert lib.bdpt_motion_query(None, C.byref(d), None) == -1
    assert lib.bdpt_gbuffer_execute_motion(None, C.byref(gp), C.byref(gb), None, None) == -1
    assert lib.bdpt_bmfr_execute_motion(None, C.byref(bp), C.byref(gb), None, None, None) == -1


def test_cpp_host_has_the_motion_switch(pkg):
    """host/bdpt_render was built with --no-motion, and the host's headers offer the PrevWorldPosition switch: a snippet
    that uses BlockwiseMultiOrderFeatureRegression::setMotion and RayLaunch::requestMotion / keepPose compiles."""
    import __graft_entry__ as ge
    host = os.path.join(ge.PKG_DIR, "host")
    exe = os.path.join(host, "bdpt_render")
    assert os.path.exists(exe), "host/bdpt_render not built (run __graft_entry__.build())"
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--no-motion" in r.stderr, r.stderr
    src = ('#include "Passes.h"\n'
           "using namespace bdpt;\n"
           "bool f(RayLaunch& r, const std::vector<hipStream_t>& s) {\n"
           "  BlockwiseMultiOrderFeatureRegression::SharedPtr p = BlockwiseMultiOrderFeatureRegression::create();\n"
           "  p->setMotion(true);\n"
           "  return r.requestMotion() && r.motion() && r.keepPose(s, 0);\n"
           "}\n")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "motion_switch.cpp")
        open(c, "w").write(src)
        cc = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", host, c],
                            capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    passes = open(os.path.join(host, "Passes.cpp")).read()
    assert "PrevWorldPosition" in passes and "bdpt_gbuffer_execute_motion" in passes and "bdpt_bmfr_execute_motion" in passes
