"""CPU checks of area lights (include/bdpt.h "Area lights"): the entry points are declared, exported and bound, the info
struct matches the header, the NULL-argument errors need no device, and the float64 numpy restatement
(area_light_numpy.py) gets weights, CDF, selection and pdf right on a hand-built mesh."""
import ctypes as C
import math
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np

from area_light_numpy import AreaTable, CHANNEL_CONST, CHANNEL_TEXTURE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "bdpt.h")


def test_area_light_entry_points_declared_exported_and_bound(pkg):
    hdr = open(HDR).read()
    a = pkg.abi
    for name, const in (("BDPT_PARAM_AREA_LIGHTS", a.PARAM_AREA_LIGHTS), ("BDPT_PREPARE_AREA_LIGHTS", a.PREPARE_AREA_LIGHTS)):
        m = re.search(rf"#define {name} (\d+)u", hdr)
        assert m and int(m.group(1)) == const, name
    assert a.PARAM_AREA_LIGHTS == 4096 and a.PREPARE_AREA_LIGHTS == 16
    other = [getattr(a, n) for n in dir(a) if n.startswith("PARAM_") and n != "PARAM_AREA_LIGHTS"]
    assert all(a.PARAM_AREA_LIGHTS & o == 0 for o in other)
    so = os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "csrc", "libbdpt_amd.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    lib = pkg.load_library()
    for name, nargs in (("bdpt_get_area_light_info", 2), ("bdpt_test_area_light_sample", 6)):
        m = re.search(rf"int {name}\(([^)]*)\);", hdr)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert re.search(rf"\bT {name}$", syms, flags=re.M), name
        res, args = a.PROTOTYPES[name]
        assert res is C.c_int and len(args) == nargs
        assert getattr(lib, name).argtypes == args


def test_area_light_info_struct_matches_header(pkg):
    hdr = open(HDR).read()
    body = re.search(r"typedef struct bdpt_area_light_info \{(.*?)\} bdpt_area_light_info;", hdr, re.S).group(1)
    fields = re.findall(r"(uint32_t|float) (\w+);", body)
    assert [f for _, f in fields] == [f for f, _ in pkg.abi.AreaLightInfo._fields_]
    assert C.sizeof(pkg.abi.AreaLightInfo) == 16


def test_null_arguments_need_no_device(pkg):
    lib = pkg.load_library()
    info = pkg.abi.AreaLightInfo()
    assert lib.bdpt_get_area_light_info(None, C.byref(info)) == -1
    assert lib.bdpt_test_area_light_sample(None, 0, None, None, 0, None) == -1


def _mat(emissive, typ, tex=-1):
    flags = (CHANNEL_CONST << 3) | (typ << 9)
    return SimpleNamespace(emissive=list(emissive), flags=flags, texEmissive=tex, texBaseColor=-1, alphaThreshold=0.5,
                           baseColor=[0.5, 0.5, 0.5, 1.0])


def _mesh():
    """four triangles: a 2x1 right triangle (constant emitter), a dark one (not an emitter), a textured emitter, and a
    degenerate constant emitter (zero area)"""
    P = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0],
                  [0, 0, 1], [1, 0, 1], [0, 1, 1],
                  [0, 0, 2], [3, 0, 2], [0, 3, 2],
                  [0, 0, 3], [1, 0, 3], [2, 0, 3]], np.float64)
    I = np.arange(12).reshape(4, 3)
    mats = [_mat((1.0, 1.0, 1.0), CHANNEL_CONST), _mat((0.0, 0.0, 0.0), CHANNEL_CONST), _mat((0, 0, 0), CHANNEL_TEXTURE, 0),
            _mat((2.0, 0.0, 0.0), CHANNEL_CONST)]
    return P, I, np.arange(4), mats


def test_weights_cdf_and_pdf_on_a_hand_built_mesh():
    P, I, M, mats = _mesh()
    tex = (np.full((2, 2, 4), 255, np.uint8), True)
    t = AreaTable(P, I, M, mats, [tex])
    assert list(t.prim) == [0, 2, 3]  # ascending; the black triangle is no emitter
    assert np.allclose(t.area, [1.0, 4.5, 0.0])
    lam0 = 0.2126 + 0.7152 + 0.0722
    assert np.allclose(t.w, [1.0 * lam0, 4.5 * 1.0, 0.0])  # textured: lambda = 1; degenerate: weight 0
    assert np.allclose(t.cdf, np.cumsum(t.w)) and t.W == t.cdf[-1]
    assert t.last == 1
    # selection: the first CDF entry > a W; the zero-weight emitter is never picked
    assert t.pick(0.0) == 0 and t.pick(t.cdf[0] / t.W) == 1 and t.pick(0.999999) == 1 and t.pick(1.0) == 1
    # p_A = w_i / (W area_i): for a constant emitter lambda_i / W, everywhere on it
    assert math.isclose(t.pdf_area(0), lam0 / t.W) and math.isclose(t.pdf_area(1), 1.0 / t.W)
    # the pdf integrates to one over the emitters with weight
    assert math.isclose(t.pdf_area(0) * t.area[0] + t.pdf_area(1) * t.area[1], 1.0)


def test_point_sampling_is_uniform_on_the_triangle_and_follows_the_weights():
    P, I, M, mats = _mesh()
    t = AreaTable(P, I, M, mats, [(np.full((2, 2, 4), 255, np.uint8), True)])
    rng = np.random.default_rng(3)
    u = rng.random((20000, 3))
    pts = [t.point(*r) for r in u]
    frac = np.mean([p["i"] == 1 for p in pts])
    assert abs(frac - t.w[1] / t.W) < 0.015
    on0 = np.array([p["pos"] for p in pts if p["i"] == 0])
    assert (on0[:, 0] >= 0).all() and (on0[:, 1] >= 0).all() and (on0[:, 0] / 2 + on0[:, 1] <= 1 + 1e-12).all()
    assert abs(on0[:, 0].mean() - 2 / 3) < 0.02 and abs(on0[:, 1].mean() - 1 / 3) < 0.02  # uniform: the centroid
    x = t.point(0.0, 0.25, 0.5)
    assert x["prim"] == 0 and math.isclose(x["b1"], 0.25) and math.isclose(x["b2"], 0.5)
    assert np.allclose(x["ng"], [0, 0, 1]) and np.allclose(x["Le"], [1, 1, 1])
    # textured emission: the decoded texel (white)
    y = t.point(0.99, 0.5, 0.5)
    assert y["prim"] == 2 and np.allclose(y["Le"], [1, 1, 1])


def test_nee_and_light_start_follow_the_draw_order():
    P, I, M, mats = _mesh()
    t = AreaTable(P, I, M, mats, [(np.full((2, 2, 4), 255, np.uint8), True)])
    x, L, d, inten = t.nee(12345, [0.5, 0.25, -1.0])
    assert math.isclose(float(np.linalg.norm(L)), 1.0) and d > 0
    expect = x["Le"] * abs(float(x["ng"] @ L)) / (x["pA"] * d * d)
    assert np.allclose(inten, expect)
    x, n, dirv, col, seed = t.light_start(777)
    assert abs(abs(float(n @ x["ng"])) - 1.0) < 1e-12 and float(dirv @ n) >= 0
    assert np.allclose(col, x["Le"] * 2 * math.pi / x["pA"])
    # six draws: a, u1, u2, s and the two of the cosine sample
    s = 777
    for _ in range(6):
        s = (1664525 * s + 1013904223) & 0xFFFFFFFF
    assert seed == s
    # a receiving point on the emitter's plane at distance 0 is +0
    x, L, d, inten = t.nee(1, x["pos"]) if False else t.nee(1, [0.0, 0.0, 0.0])
    assert np.isfinite(inten).all()
