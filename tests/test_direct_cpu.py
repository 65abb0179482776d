"""CPU checks of direct lighting (bdpt_direct_query, bdpt_direct_execute): the ctypes structures against include/bdpt.h, the
Python binding against a fake library, the intensity restatement of tests/direct_reference.py against oracle_light_nee bit for
bit, the oracle composition against a float64 reading of the reference's shader, the no-ray rule, dead items and the
specular fallback."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import direct_reference as dr
from binding_fakes import ROOT, FakeGpuTensor, RecordingLib, context_without_device, desc_fields, header_layout
from edge_rays import F64_MAX_LEFT_OUT

F, U = np.float32, np.uint32
MIN_T = 1e-4
STRUCTS = {
    "bdpt_direct_desc": ("DirectDesc", ["num", "flags", "numDevice", "minT", "reserved", "surfaces", "alive", "color", "visible", "traced"]),
    "bdpt_direct_params": ("DirectParams", ["minT", "flags", "reserved"]),
}


def test_direct_structs_match_the_header(pkg):
    a = pkg.abi
    lay = header_layout({c: f for c, (_, f) in STRUCTS.items()}, {"BDPT_DIRECT_USE_HINTS": ["BDPT_DIRECT_USE_HINTS"], "MAX": ["BDPT_MAX_LIGHTS"]})
    for cname, (pyname, fields) in STRUCTS.items():
        cls = getattr(a, pyname)
        assert int(lay[cname]) == C.sizeof(cls), cname
        assert [n for n, _ in cls._fields_] == fields, cname
        for name in fields:
            assert int(lay[f"{cname}.{name}"]) == getattr(cls, name).offset, (cname, name)
    assert C.sizeof(a.DirectParams) == 16 and C.sizeof(a.DirectDesc) == 64
    assert int(lay["BDPT_DIRECT_USE_HINTS"]) == a.DIRECT_USE_HINTS == dr.USE_HINTS == 1
    assert int(lay["MAX"]) == dr.MAX_LIGHTS == 16  # one mask bit per light, two masks in a word inside the kernel


def test_the_entry_points_are_declared_exported_and_bound(pkg):
    a = pkg.abi
    src = open(os.path.join(ROOT, "include", "bdpt.h")).read()
    assert re.search(r"int\s+bdpt_direct_query\(bdpt_ctx\*\s*\w+,\s*const bdpt_direct_desc\*\s*\w+,\s*void\*\s*\w+\);", src)
    assert re.search(r"int\s+bdpt_direct_execute\(bdpt_ctx\*\s*\w+,\s*const bdpt_direct_params\*\s*\w+,\s*const bdpt_gbuffer\*\s*\w+,"
                     r"\s*float\*\s*\w+,\s*void\*\s*\w+\);", src)
    assert src.index("---- Diffuse GI") < src.index("---- Direct lighting") < src.index("int bdpt_direct_query(")
    section = src[src.index("---- Direct lighting"):src.index("int bdpt_direct_query(")]
    for text in ("lambertianPlusShadows.rt.hlsl", "LambertianPlusShadowPass.cpp", "Record contract", "3.141592f", "0.00001f", "hitDist",
                 "does NOT apply", "BDPT_PARAM_AREA_LIGHTS", "bit-identical", "no accepted hit in (minT, dist)"):
        assert text in section, text
    assert a.PROTOTYPES["bdpt_direct_query"] == (C.c_int, [C.c_void_p, C.POINTER(a.DirectDesc), C.c_void_p])
    assert a.PROTOTYPES["bdpt_direct_execute"] == (C.c_int, [C.c_void_p, C.POINTER(a.DirectParams), C.POINTER(a.GBuffer), C.c_void_p, C.c_void_p])
    raw = C.CDLL(a.LIB_PATH)
    assert hasattr(raw, "bdpt_direct_query") and hasattr(raw, "bdpt_direct_execute")
    lib = pkg.load_library()
    assert lib.bdpt_direct_query.argtypes == a.PROTOTYPES["bdpt_direct_query"][1] and lib.bdpt_direct_query.restype is C.c_int
    assert lib.bdpt_direct_query(None, None, None) == -1 and lib.bdpt_direct_execute(None, None, None, None, None) == -1  # BDPT_E_INVALID


def _ctx(pkg, device=0):
    return context_without_device(pkg, RecordingLib({"bdpt_direct_query": lambda d, stream: (desc_fields(d), stream),
                                                     "bdpt_direct_execute": lambda p, gb, out, stream: (desc_fields(p), gb, out, stream)}), device)


def test_good_calls_reach_the_library(pkg):
    import torch
    ctx = _ctx(pkg)
    f32, i32, u32, u8 = torch.float32, torch.int32, torch.uint32, torch.uint8
    n = 70
    surf, alive, out = FakeGpuTensor((n, 24), f32, ptr=0x10000), FakeGpuTensor((n,), u8, ptr=0x30000), FakeGpuTensor((n, 4), f32, ptr=0x40000)
    vis, trc, cnt = FakeGpuTensor((n,), u32, ptr=0x50000), FakeGpuTensor((n,), i32, ptr=0x60000), FakeGpuTensor((1,), i32, ptr=0x80000)
    res = ctx.direct_lighting(surf, alive=alive, min_t=0.25, use_hints=True, visible=vis, traced=trc, out=out, count=cnt, stream="st")
    assert isinstance(res, tuple) and res[0] is out and res[1] is vis and res[2] is trc
    c, st = ctx._lib.calls[-1]
    assert st == "st" and c == dict(num=n, flags=1, numDevice=0x80000, minT=0.25, reserved=0, surfaces=0x10000, alive=0x30000, color=0x40000,
                                    visible=0x50000, traced=0x60000)
    res = ctx.direct_lighting(FakeGpuTensor((n, 24), i32, ptr=0x10000), min_t=1e-4, out=out)
    assert res is out
    c, st = ctx._lib.calls[-1]
    assert (c["flags"], c["minT"], st) == (0, F(1e-4), None)
    assert [c[k] for k in ("numDevice", "alive", "visible", "traced")] == [None] * 4
    res = ctx.direct_lighting(surf, min_t=1e-4, out=out, traced=trc)
    assert len(res) == 2 and res[1] is trc and ctx._lib.calls[-1][0]["visible"] is None
    ctx._frame = (2, 3)
    img, gb = FakeGpuTensor((2, 3, 4), f32, ptr=0x1234), pkg.abi.GBuffer()
    p = ctx.direct_execute(gb, img, min_t=0.5, use_hints=True, stream="stream")
    fields, gb_seen, out_seen, st = ctx._lib.calls[-1]
    assert fields == dict(minT=0.5, flags=1, reserved=[0, 0]) and gb_seen is gb and (out_seen.value, st) == (0x1234, "stream")
    assert isinstance(p, pkg.abi.DirectParams) and p.flags == 1
    ctx.direct_execute(gb, img, min_t=0.5)
    assert ctx._lib.calls[-1][0]["flags"] == 0


def test_bad_arguments_are_refused_before_the_library(pkg):
    import torch
    ctx = _ctx(pkg)
    f32, i32, u32, u8 = torch.float32, torch.int32, torch.uint32, torch.uint8
    n = 64
    good = dict(surfaces=FakeGpuTensor((n, 24), f32), min_t=1e-4)
    bad = [
        dict(good, surfaces=FakeGpuTensor((n, 24), f32, index=1)), dict(good, surfaces=FakeGpuTensor((n, 20), f32)),
        dict(good, surfaces=FakeGpuTensor((n, 24), torch.float64)), dict(good, surfaces=FakeGpuTensor((n, 24), f32, contiguous=False)),
        dict(good, alive=FakeGpuTensor((n,), torch.bool)), dict(good, alive=FakeGpuTensor((n + 1,), u8)), dict(good, alive=torch.zeros(n, dtype=u8)),
        dict(good, out=FakeGpuTensor((n,), f32)), dict(good, out=FakeGpuTensor((n, 3), f32)), dict(good, out=FakeGpuTensor((n, 4), i32)),
        dict(good, out=torch.zeros(n, 4)), dict(good, visible=FakeGpuTensor((n,), f32)), dict(good, visible=FakeGpuTensor((n - 1,), u32)),
        dict(good, visible=None), dict(good, visible=1), dict(good, traced=FakeGpuTensor((n, 1), u32)),
        dict(good, traced=FakeGpuTensor((n,), u32, contiguous=False)), dict(good, traced=torch.zeros(n, dtype=i32)),
        dict(good, count=FakeGpuTensor((2,), u32)), dict(good, count=FakeGpuTensor((1,), torch.int64)), dict(good, count=torch.ones(1, dtype=i32)),
        dict(surfaces=np.zeros((n, 24), F), min_t=1e-4, visible=FakeGpuTensor((n,), u32)),  # host arrays take no output tensors
        dict(surfaces=np.zeros((n, 24), F), min_t=1e-4, traced=True), dict(surfaces=np.zeros((n, 20), F), min_t=1e-4),
    ]
    for kw in bad:
        with pytest.raises(pkg.BdptError):
            ctx.direct_lighting(**kw)
    with pytest.raises(TypeError):
        ctx.direct_lighting(good["surfaces"])  # min_t is required: there is no default tmin
    with pytest.raises(TypeError):
        ctx.direct_lighting(good["surfaces"], None, min_t=1e-4)  # everything after the records goes by keyword
    gb, img = pkg.abi.GBuffer(), FakeGpuTensor((2, 3, 4), f32)
    with pytest.raises(pkg.BdptError):
        ctx.direct_execute(gb, img, min_t=1e-4)  # no frame size yet
    ctx._frame = (2, 3)
    for g, o in ((None, img), (gb, FakeGpuTensor((2, 3, 3), f32)), (gb, FakeGpuTensor((2, 3, 4), torch.float16)), (gb, torch.zeros(2, 3, 4)),
                 (gb, FakeGpuTensor((2, 3, 4), f32, index=1))):
        with pytest.raises(pkg.BdptError):
            ctx.direct_execute(g, o, min_t=1e-4)
    assert ctx._lib.calls == []


def test_frame_pipeline_direct_lighting_passes_its_settings(pkg):
    """FramePipeline.direct_lighting hands Context.direct_execute the pipeline's min_t, G-buffer, channel and stream, and the
    hint switch; a use_hints that is no bool is refused before the context is reached"""
    import torch
    seen = []

    class Ctx:
        def direct_execute(self, gb, out, *, min_t, use_hints=False, stream=None):
            seen.append((gb, out, min_t, use_hints, stream))
            return "params"

    pipe = pkg.FramePipeline.__new__(pkg.FramePipeline)
    pipe.ctx, pipe.min_t, pipe.gb, pipe.last_direct_params = Ctx(), 0.5, "gb", None
    pipe.channels = {pkg.DIRECT_CHANNEL: FakeGpuTensor((2, 3, 4), torch.float32, ptr=0x5000)}
    pipe._stream_ptr = lambda: "stream"
    out = pipe.direct_lighting()
    assert out is pipe.channels[pkg.DIRECT_CHANNEL] and pkg.DIRECT_CHANNEL == "DirectLighting"
    assert seen[-1] == ("gb", out, 0.5, False, "stream") and pipe.last_direct_params == "params"
    pipe.direct_lighting(use_hints=True)
    assert seen[-1][3] is True
    for bad in (1, None, "yes"):
        with pytest.raises(pkg.BdptError):
            pipe.direct_lighting(use_hints=bad)
    assert len(seen) == 2


# ---- the CPU yardstick ---------------------------------------------------------------------------------------------------
class _Case:
    def __init__(self, pkg, ob, name):
        self.lib = ob.load_oracle(pkg.abi)
        self.sc = {"room": dr.DirectScene, "three": dr.three_light_scene, "sixteen": dr.sixteen_light_scene}[name](pkg)
        self.osc = self.lib.oracle_scene_create(C.byref(self.sc.desc))
        assert self.osc
        self.backend = dr.OracleBackend(ob, pkg.abi, self.lib, self.osc, self.sc.lights, MIN_T)

    def close(self):
        self.lib.oracle_scene_destroy(self.osc)


SCENES = ("room", "three", "sixteen")


@pytest.fixture(scope="module")
def cases(pkg, ob):
    cs = {name: _Case(pkg, ob, name) for name in SCENES}
    yield cs
    for c in cs.values():
        c.close()


def _edge_positions(lights, rec):
    """positions at, and within sqrt(1e-5) of, the lights, into every 16th record"""
    rec = rec.copy()
    for j, i in enumerate(range(0, len(rec), 16)):
        lt = lights[j % len(lights)]
        lp = np.array([lt.posW[k] for k in range(3)], F)
        rec[i, 0:3] = lp + (np.array([0.002, -0.001, 0.001], F) if j % 2 else F(0))
    return rec


@pytest.mark.parametrize("name", SCENES)
def test_intensity_restatement_equals_oracle_light_nee(pkg, ob, cases, name):
    """on records with diffuse = (1, 1, 1), for every (item, light) pair of the scene: (((1 * LdotN) * I) * 1) / kPi with the
    restatement's I equals oracle_light_nee's value on the one-light table bit for bit (two NaNs equal); L and dist of the
    restatement equal the oracle's too.  Items at a light and within sqrt(1e-5) of it are among them."""
    c = cases[name]
    rec = _edge_positions(c.sc.lights, c.sc.records(np.random.default_rng(5), 4096))
    rec[:, 12:15] = 1.0
    rec[::5, 4:7] *= F(0.7)  # N need not be unit
    lit = 0
    for k in range(len(c.sc.lights)):
        smp, _ = ob.light_nee(pkg.abi, dr.one_light(pkg.abi, c.sc.lights, k), rec, np.zeros(len(rec), U), 1, MIN_T)
        L, inten, dist = dr.light_intensity(c.sc.lights[k], rec[:, 0:3])
        assert dr.same_bits(L, smp[:, 4:7]).all() and dr.same_bits(dist, smp[:, 7]).all(), (name, k)
        with np.errstate(all="ignore"):
            ldn = dr.saturate(dr.dot3(rec[:, 4:7], smp[:, 4:7]))
        want = dr.pin_value(ldn, inten)
        bad = ~dr.same_bits(want, smp[:, 8:11]).all(axis=1)
        assert not bad.any(), (name, k, int(bad.sum()), np.nonzero(bad)[0][:4])
        lit += int((smp[:, 8:11] > 0).any(axis=1).sum())
    assert lit > len(rec) // 4


@pytest.mark.parametrize("name", SCENES)
def test_oracle_composition_against_a_float64_reading(pkg, ob, cases, name):
    """direct_oracle against direct_f64 on 2048 surface points and 16 miss records: every colour within 1e-4 relative plus 1e-6
    absolute, but for the items left out: a ray within F64_TOL of an edge or an interval end, cosTheta within 1e-6 of a cone,
    dot(dif, dif) within 1e-7 of 0.00001.  At most 2 % are left out.  Measured (edge / cone / fallback of 2064): room 0 / 0 / 0,
    three lights 1 / 0 / 0, sixteen lights 6 / 0 / 0: 0.00 %, 0.05 % and 0.29 %."""
    c = cases[name]
    n = 2048
    rec = c.sc.records(np.random.default_rng(41), n, misses=16)
    got = dr.direct_compose(c.backend, rec, MIN_T)
    ref = dr.direct_f64(c.sc, rec, MIN_T)
    left = np.zeros(len(rec), bool)
    for mask in ref["left_out"].values():
        left |= mask
    counts = {k: int(v.sum()) for k, v in ref["left_out"].items()}
    print(f"{name}: left out {counts} of {len(rec)}: {100.0 * left.mean():.2f} %")
    assert left.mean() <= F64_MAX_LEFT_OUT, counts
    c32, c64 = got["color"][:, 0:3].astype(np.float64), ref["color"]
    bad = (np.abs(c32 - c64) > 1e-4 * np.abs(c64) + 1e-6).any(axis=1) & ~left
    assert not bad.any(), (int(bad.sum()), np.nonzero(bad)[0][:8], c32[bad][:2], c64[bad][:2])
    assert np.array_equal(got["live"], ref["live"]) and (got["color"][:, 3] == 1.0).all() and np.isfinite(c32).all()
    lv = got["live"]
    assert 0 < (c32[lv].max(axis=1) > 0).mean() and (got["traced"][lv] != 0).any()
    full = U((1 << len(c.sc.lights)) - 1)
    assert ((got["visible"][lv] & full) != full).any(), "no occluded light: the scene shadows nothing"
    assert (got["visible"] & ~full == 0).all() and (got["traced"] & ~full == 0).all()


class _Constant:
    """a backend whose any_hit answers one value: the no-ray rule"""

    def __init__(self, inner, answer):
        self.inner, self.answer, self.num_lights = inner, answer, inner.num_lights
        self.light_ray, self.intensity = inner.light_ray, inner.intensity

    def any_hit(self, rays):
        return np.full(len(rays), self.answer, bool)


def test_no_ray_where_it_cannot_change_a_bit(pkg, ob, cases):
    """for (item, light) pairs with LdotN == 0 or I == 0 the term has the same bits whether the ray is called visible or
    occluded, also for the non-finite and negative intensities: so items ALL of whose pairs are such have the same colour,
    and every item's `traced` mask is what the rule says"""
    c = cases["sixteen"]
    rec = _edge_positions(c.sc.lights, c.sc.records(np.random.default_rng(9), 1024))
    rec[::9, 4:7] = np.negative(rec[::9, 4:7])  # facing away from most lights
    rec[5::32, 4:7] = np.array([np.nan, 0, 1], F)
    rec[7::32, 4:7] = 0
    a = dr.direct_compose(_Constant(c.backend, True), rec, MIN_T, trace_all=True)
    b = dr.direct_compose(_Constant(c.backend, False), rec, MIN_T, trace_all=True)
    plain = dr.direct_compose(_Constant(c.backend, False), rec, MIN_T)
    assert np.array_equal(a["traced"], b["traced"]) and np.array_equal(a["traced"], plain["traced"])
    none = a["traced"] == 0
    assert none.sum() > 64 and (~none).sum() > 64
    assert dr.same_bits(a["color"][none], b["color"][none]).all()
    assert not dr.same_bits(a["color"][~none], b["color"][~none]).all(axis=1).all()
    # asking for the rays the rule leaves out changes nothing: the plain composition is the all-rays one
    assert dr.same_bits(plain["color"], b["color"]).all()
    # per pair: (0 * LdotN) * I and (1 * LdotN) * I are the same bits where no ray is needed
    with np.errstate(all="ignore"):
        for k in range(c.backend.num_lights):
            skip = ~a["need"][k] & a["live"]
            ldn, inten = a["ldn"][k][skip], a["inten"][k][skip]
            assert dr.same_bits((F(0) * ldn)[:, None] * inten, (F(1) * ldn)[:, None] * inten).all(), k
    # and with extreme intensities: inf, -inf, NaN, negative, zero
    lights = dr.sixteen_lights(pkg.abi)
    for k, val in enumerate((np.inf, -np.inf, np.nan, -2.0, 0.0, -0.0)):
        lights[k].intensity[0] = val
    q = dr.OracleBackend(ob, pkg.abi, c.lib, c.osc, lights, MIN_T)
    with np.errstate(all="ignore"):
        a = dr.direct_compose(_Constant(q, True), rec, MIN_T, trace_all=True)
        b = dr.direct_compose(_Constant(q, False), rec, MIN_T, trace_all=True)
        for k in range(6):
            skip = ~a["need"][k] & a["live"]
            assert skip.any()
            ldn, inten = a["ldn"][k][skip], a["inten"][k][skip]
            assert dr.same_bits((F(0) * ldn)[:, None] * inten, (F(1) * ldn)[:, None] * inten).all(), k
    none = a["traced"] == 0
    assert dr.same_bits(a["color"][none], b["color"][none]).all()
    assert np.isnan(b["color"][~none]).any(), "an occluded light of infinite intensity is 0 * inf = NaN: the shader multiplies"


def test_dead_items_and_the_specular_fallback(pkg, ob, cases):
    """a dead item (prim < 0, or alive == 0) shows (dif, 1) after the fallback with both masks 0; dot(dif, dif) one step
    below 0.00001 takes the specular colour, at and above it keeps the diffuse one, and a NaN diffuse keeps itself"""
    c = cases["three"]
    rec = c.sc.records(np.random.default_rng(3), 512, misses=32, dead_run=(100, 40))
    x = np.sqrt(np.float64(1e-5))
    lo, hi = F(x), F(x)
    while F(lo * lo) >= dr.FALLBACK:
        lo = np.nextafter(lo, F(0))
    while F(hi * hi) < dr.FALLBACK:
        hi = np.nextafter(hi, F(1))
    assert F(lo * lo) < dr.FALLBACK <= F(hi * hi)
    rec[0:8, 12:15] = 0
    rec[0:4, 12], rec[4:8, 12] = lo, hi
    rec[8, 12:15] = (np.nan, 0, 0)
    rec[200:204, 12:15] = 0
    rec[200:202, 13], rec[202:204, 13] = lo, hi
    rec.view(np.int32)[200:204, 23] = -2
    alive = (np.arange(len(rec)) % 5 != 0).astype(np.uint8)
    got = dr.direct_compose(c.backend, rec, MIN_T, alive=alive)
    dead = (rec.view(np.int32)[:, 23] < 0) | (alive == 0)
    assert np.array_equal(got["live"], ~dead) and dead.sum() > 72
    alb = dr.albedo(rec)
    assert dr.same_bits(alb[0:4], rec[0:4, 16:19]).all() and dr.same_bits(alb[4:8], rec[4:8, 12:15]).all()
    assert dr.same_bits(alb[8], rec[8, 12:15]).all()
    assert dr.same_bits(alb[200:202], rec[200:202, 16:19]).all() and dr.same_bits(alb[202:204], rec[202:204, 12:15]).all()
    assert dr.same_bits(got["color"][dead, 0:3], alb[dead]).all() and (got["color"][:, 3] == 1.0).all()
    assert (got["visible"][dead] == 0).all() and (got["traced"][dead] == 0).all()
    lv = got["live"]
    # an alive item with the fallback is lit through its specular colour
    j = np.nonzero(lv & (np.arange(len(rec)) < 4))[0]
    assert len(j) and (got["color"][j, 0:3] > 0).any()


# ---- the host pass -------------------------------------------------------------------------------------------------------
def test_direct_pass_compiles_under_its_reference_name():
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    host = os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "host")
    src = os.path.join(ROOT, "tests", "host_compile", "direct_pass_main.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + host, src],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "using namespace" not in open(src).read().split("int main")[1]
    names = open(os.path.join(host, "ReferenceNames.h")).read()
    assert "using bdpt::LambertianPlusShadowPass;" in names


def test_bdpt_render_refuses_bad_direct_options():
    """--direct-hints without --direct, --direct with --gpus / --world / --ao / --gi, and the switches only the replaced
    passes read exit non-zero with a message, before any GPU is touched"""
    import subprocess
    render = os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "host", "bdpt_render")
    if not os.path.exists(render):
        pytest.skip("host/bdpt_render not built")
    for args, text in ((["--direct-hints"], "goes with --direct"), (["--direct", "--gpus", "1"], "one GPU"),
                       (["--direct", "--world", "2", "--rank", "0"], "one GPU"), (["--direct", "--ao", "4"], "not together with --ao"),
                       (["--direct", "--gi"], "not together with --ao N or --gi"), (["--direct", "--denoise"], "not with --denoise"),
                       (["--direct", "--area-lights"], "not with --denoise"), (["--direct", "--no-motion"], "not with --denoise")):
        r = subprocess.run([render] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and text in r.stderr, (args, r.stderr)
    u = subprocess.run([render, "--help"], capture_output=True, text=True, timeout=60)
    assert "--direct [--direct-hints]" in u.stderr
