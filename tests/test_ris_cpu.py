"""CPU checks of resampled direct lighting (bdpt_ris_query, bdpt_ris_execute): the ctypes structures against include/bdpt.h,
the Python binding against a fake library, and the definition (tests/ris_reference.py ris_compose over the CPU oracle): one
candidate is plain next-event estimation bit for bit, and the estimator is unbiased against an enumeration of the lights."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import direct_reference as dr
import ris_reference as rr
from binding_fakes import ROOT, FakeGpuTensor, RecordingLib, context_without_device, desc_fields, header_layout

F, U = np.float32, np.uint32
MIN_T = 1e-4
STRUCTS = {
    "bdpt_ris_desc": ("RisDesc", ["num", "flags", "numDevice", "matIndex", "candidates", "samples", "clampUpper", "minT", "reserved",
                                  "surfaces", "alive", "seeds", "color", "seedsOut", "traced", "reservoirs"]),
    "bdpt_ris_params": ("RisParams", ["frameCount", "clampUpper", "minT", "candidates", "samples", "matIndex", "flags", "reserved"]),
    "bdpt_ris_reservoir": ("RisReservoir", ["light", "status", "state", "W", "wsum"]),
}


def test_ris_structs_match_the_header(pkg):
    a = pkg.abi
    consts = {"FLAGS": ["BDPT_RIS_USE_HINTS", "BDPT_PARAM_AREA_LIGHTS"], "MAX": ["BDPT_RIS_MAX_CANDIDATES", "BDPT_RIS_MAX_SAMPLES"],
              "STATUS": ["BDPT_RIS_STATUS_RAY", "BDPT_RIS_STATUS_HINT_OCCLUDED", "BDPT_RIS_STATUS_OCCLUDED", "BDPT_RIS_NO_LIGHT"]}
    lay = header_layout({c: f for c, (_, f) in STRUCTS.items()}, consts)
    for cname, (pyname, fields) in STRUCTS.items():
        cls = getattr(a, pyname)
        assert int(lay[cname]) == C.sizeof(cls), cname
        assert [n for n, _ in cls._fields_] == fields, cname
        for name in fields:
            assert int(lay[f"{cname}.{name}"]) == getattr(cls, name).offset, (cname, name)
    assert [C.sizeof(getattr(a, n)) for n in ("RisDesc", "RisParams", "RisReservoir")] == [96, 32, 16]
    assert [int(v) for v in lay["FLAGS"].split()] == [a.RIS_USE_HINTS, a.PARAM_AREA_LIGHTS] == [rr.USE_HINTS, 4096]
    assert [int(v) for v in lay["MAX"].split()] == [a.RIS_MAX_CANDIDATES, a.RIS_MAX_SAMPLES] == [32, 64]
    assert [int(v) for v in lay["STATUS"].split()] == [a.RIS_STATUS_RAY, a.RIS_STATUS_HINT_OCCLUDED, a.RIS_STATUS_OCCLUDED, a.RIS_NO_LIGHT] \
        == [rr.STATUS_RAY, rr.STATUS_HINT_OCCLUDED, rr.STATUS_OCCLUDED, rr.NO_LIGHT]


def test_the_entry_points_are_declared_exported_and_bound(pkg):
    a = pkg.abi
    src = open(os.path.join(ROOT, "include", "bdpt.h")).read()
    assert re.search(r"int\s+bdpt_ris_query\(bdpt_ctx\*\s*\w+,\s*const bdpt_ris_desc\*\s*\w+,\s*void\*\s*\w+\);", src)
    assert re.search(r"int\s+bdpt_ris_execute\(bdpt_ctx\*\s*\w+,\s*const bdpt_ris_params\*\s*\w+,\s*const bdpt_gbuffer\*\s*\w+,"
                     r"\s*float\*\s*\w+,\s*void\*\s*\w+\);", src)
    section = src[src.index("---- Resampled direct lighting"):src.index("int bdpt_ris_query(")]
    for text in ("u_c * wsum <= w_c", "(wsum / (float)candidates) / w_sel", "always taken", "BDPT_E_STATE", "areaNee(state)", "unbiased"):
        assert text in section, text
    assert a.PROTOTYPES["bdpt_ris_query"] == (C.c_int, [C.c_void_p, C.POINTER(a.RisDesc), C.c_void_p])
    assert a.PROTOTYPES["bdpt_ris_execute"] == (C.c_int, [C.c_void_p, C.POINTER(a.RisParams), C.POINTER(a.GBuffer), C.c_void_p, C.c_void_p])
    raw = C.CDLL(a.LIB_PATH)
    assert hasattr(raw, "bdpt_ris_query") and hasattr(raw, "bdpt_ris_execute")
    lib = pkg.load_library()
    assert lib.bdpt_ris_query(None, None, None) == -1 and lib.bdpt_ris_execute(None, None, None, None, None) == -1  # BDPT_E_INVALID
    mk = open(os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "csrc", "Makefile")).read()
    assert " ris.o " in mk and "device_light.hpp" in mk
    # one text for a candidate: both kernels call the helper, neither restates it
    csrc = os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "csrc")
    for name in ("ris.hip", "light_query.hip"):
        code = "\n".join(line.split("//")[0] for line in open(os.path.join(csrc, name)).read().splitlines())
        assert "lightCandidate<" in code and "areaNee(" not in code and "directIfVisible<" not in code, name


def _ctx(pkg, device=0):
    return context_without_device(pkg, RecordingLib({"bdpt_ris_query": lambda d, stream: (desc_fields(d), stream),
                                                     "bdpt_ris_execute": lambda p, gb, out, stream: (desc_fields(p), gb, out, stream)}), device)


def test_good_calls_reach_the_library(pkg):
    import torch
    ctx = _ctx(pkg)
    f32, i32, u32, u8 = torch.float32, torch.int32, torch.uint32, torch.uint8
    n = 70
    surf, seeds, alive = FakeGpuTensor((n, 24), f32, ptr=0x10000), FakeGpuTensor((n,), u32, ptr=0x20000), FakeGpuTensor((n,), u8, ptr=0x30000)
    out, so, trc = FakeGpuTensor((n, 4), f32, ptr=0x40000), FakeGpuTensor((n,), i32, ptr=0x50000), FakeGpuTensor((n,), u32, ptr=0x60000)
    rsv, cnt = FakeGpuTensor((n, 3, 4), i32, ptr=0x70000), FakeGpuTensor((1,), i32, ptr=0x80000)
    res = ctx.ris_lighting(surf, seeds, 8, 3, mat_index=0, area_lights=True, use_hints=True, clamp=2.5, min_t=0.25, alive=alive, out=out,
                           seeds_out=so, traced=trc, reservoirs=rsv, count=cnt, stream="st")
    assert res is out
    c, st = ctx._lib.calls[-1]
    assert st == "st" and c == dict(num=n, flags=4097, numDevice=0x80000, matIndex=0, candidates=8, samples=3, clampUpper=2.5, minT=0.25,
                                    reserved=0, surfaces=0x10000, alive=0x30000, seeds=0x20000, color=0x40000, seedsOut=0x50000,
                                    traced=0x60000, reservoirs=0x70000)
    ctx.ris_lighting(surf, seeds, 1, out=out)
    c, st = ctx._lib.calls[-1]
    assert (c["flags"], c["matIndex"], c["candidates"], c["samples"], c["clampUpper"], c["minT"], st) == (0, 1, 1, 1, F(rr.FLT_MAX), F(1e-4), None)
    assert [c[k] for k in ("numDevice", "alive", "seedsOut", "traced", "reservoirs")] == [None] * 5
    ctx._frame = (2, 3)
    img, gb = FakeGpuTensor((2, 3, 4), f32, ptr=0x1234), pkg.abi.GBuffer()
    p = ctx.ris_execute(gb, img, candidates=4, samples=2, mat_index=0, use_hints=True, clamp=1.0, min_t=0.5, frame_count=7, stream="stream")
    fields, gb_seen, out_seen, st = ctx._lib.calls[-1]
    assert fields == dict(frameCount=7, clampUpper=1.0, minT=0.5, candidates=4, samples=2, matIndex=0, flags=1, reserved=0)
    assert gb_seen is gb and (out_seen.value, st) == (0x1234, "stream") and isinstance(p, pkg.abi.RisParams)


def test_bad_arguments_are_refused_before_the_library(pkg):
    import torch
    ctx = _ctx(pkg)
    f32, i32, u32, u8 = torch.float32, torch.int32, torch.uint32, torch.uint8
    n = 64
    good = dict(surfaces=FakeGpuTensor((n, 24), f32), seeds=FakeGpuTensor((n,), u32), candidates=4)
    bad = [
        dict(good, candidates=0), dict(good, candidates=33), dict(good, candidates=True), dict(good, candidates=2.0),
        dict(good, samples=0), dict(good, samples=65), dict(good, samples=None),
        dict(good, mat_index=2), dict(good, mat_index=True), dict(good, area_lights=1), dict(good, use_hints="yes"),  # no unknown flag
        dict(good, clamp=-1.0), dict(good, clamp=float("nan")), dict(good, clamp=None),
        dict(good, surfaces=FakeGpuTensor((n, 20), f32)), dict(good, surfaces=FakeGpuTensor((n, 24), f32, contiguous=False)),
        dict(good, surfaces=FakeGpuTensor((n, 24), f32, index=1)), dict(good, seeds=FakeGpuTensor((n,), f32)),
        dict(good, seeds=FakeGpuTensor((n + 1,), u32)), dict(good, seeds=np.zeros(n, U)),
        dict(good, alive=FakeGpuTensor((n,), torch.bool)), dict(good, alive=torch.zeros(n, dtype=u8)),
        dict(good, out=FakeGpuTensor((n, 3), f32)), dict(good, out=torch.zeros(n, 4)),
        dict(good, seeds_out=FakeGpuTensor((n,), f32)), dict(good, traced=FakeGpuTensor((n, 1), u32)),
        dict(good, traced=torch.zeros(n, dtype=i32)), dict(good, reservoirs=FakeGpuTensor((n, 4), u32)),
        dict(good, samples=2, reservoirs=FakeGpuTensor((n, 1, 4), u32)), dict(good, reservoirs=FakeGpuTensor((n, 1, 4), f32)),
        dict(good, reservoirs=torch.zeros(n, 1, 4, dtype=i32)), dict(good, count=FakeGpuTensor((2,), u32)),
        dict(surfaces=np.zeros((n, 24), F), seeds=np.zeros(n, U), candidates=4, traced=FakeGpuTensor((n,), u32)),
        dict(surfaces=np.zeros((n, 24), F), seeds=np.zeros(n, U), candidates=4, reservoirs=FakeGpuTensor((n, 1, 4), u32)),
    ]
    for kw in bad:
        with pytest.raises(pkg.BdptError):
            ctx.ris_lighting(**kw)
    gb, img = pkg.abi.GBuffer(), FakeGpuTensor((2, 3, 4), f32)
    with pytest.raises(pkg.BdptError):
        ctx.ris_execute(gb, img, candidates=4)  # no frame size yet
    ctx._frame = (2, 3)
    for kw in (dict(candidates=0), dict(candidates=4, samples=65), dict(candidates=4, mat_index=3), dict(candidates=4, clamp=-0.5),
               dict(candidates=4, clamp=float("nan")), dict(candidates=4, area_lights=None)):
        with pytest.raises(pkg.BdptError):
            ctx.ris_execute(gb, img, **kw)
    for g, o in ((None, img), (gb, FakeGpuTensor((2, 3, 3), f32)), (gb, torch.zeros(2, 3, 4)), (gb, FakeGpuTensor((2, 3, 4), f32, index=1))):
        with pytest.raises(pkg.BdptError):
            ctx.ris_execute(g, o, candidates=4)
    with pytest.raises(TypeError):
        ctx.ris_execute(gb, img)  # candidates is required
    assert ctx._lib.calls == []


def test_frame_pipeline_ris_lighting_passes_its_settings(pkg):
    """FramePipeline.ris_lighting hands Context.ris_execute the pipeline's min_t, G-buffer, channel and stream, and a frame
    counter of its own that starts at 0 and advances by one per call"""
    import torch
    seen = []

    class Ctx:
        def ris_execute(self, gb, out, **kw):
            seen.append((gb, out, kw))
            return "params"

    pipe = pkg.FramePipeline.__new__(pkg.FramePipeline)
    pipe.ctx, pipe.min_t, pipe.gb, pipe.last_ris_params, pipe.ris_frame = Ctx(), 0.5, "gb", None, 0
    pipe.channels = {pkg.RIS_CHANNEL: FakeGpuTensor((2, 3, 4), torch.float32, ptr=0x5000)}
    pipe._stream_ptr = lambda: "stream"
    out = pipe.ris_lighting(8)
    assert out is pipe.channels[pkg.RIS_CHANNEL] and pkg.RIS_CHANNEL == "ResampledDirect" and pipe.last_ris_params == "params"
    assert seen[-1] == ("gb", out, dict(candidates=8, samples=1, mat_index=1, area_lights=False, use_hints=False, clamp=rr.FLT_MAX, min_t=0.5,
                                        frame_count=0, stream="stream"))
    pipe.ris_lighting(4, samples=2, mat_index=0, area_lights=True, use_hints=True, clamp=3.0)
    assert seen[-1][2] == dict(candidates=4, samples=2, mat_index=0, area_lights=True, use_hints=True, clamp=3.0, min_t=0.5, frame_count=1,
                               stream="stream") and pipe.ris_frame == 2


# ---- the definition over the CPU oracle ------------------------------------------------------------------------------------
class _Case:
    def __init__(self, pkg, ob, name):
        self.lib = ob.load_oracle(pkg.abi)
        self.sc = {"three": dr.three_light_scene, "sixteen": dr.sixteen_light_scene}[name](pkg)
        self.osc = self.lib.oracle_scene_create(C.byref(self.sc.desc))
        assert self.osc

    def backend(self, pkg, ob, mat):
        return rr.OracleBackend(ob, pkg.abi, self.lib, self.osc, self.sc.lights, mat, MIN_T)

    def close(self):
        self.lib.oracle_scene_destroy(self.osc)


@pytest.fixture(scope="module")
def cases(pkg, ob):
    cs = {name: _Case(pkg, ob, name) for name in ("three", "sixteen")}
    yield cs
    for c in cs.values():
        c.close()


def test_next_rand_is_the_reference_generator():
    rr.pin_next_rand(np.array([0, 1, 0xFFFFFFFF, 0x80000000, 12345, 0xDEADBEEF], U))
    rr.pin_next_rand(np.random.default_rng(1).integers(0, 2**32, 256, dtype=np.uint64).astype(U))


@pytest.mark.parametrize("mat", [1, 0])
def test_one_candidate_is_plain_next_event_estimation(pkg, ob, cases, mat):
    """(1) ris_compose over the oracle with M = 1, K = 1 equals oracle_light_nee's value masked by oracle_trace, bit for bit
    (clampVec at FLT_MAX: NaN and negative components +0), and the state has advanced twice: the second draw is taken"""
    c = cases["sixteen"]
    rng = np.random.default_rng(11)
    rec = rr.with_view(c.sc.records(rng, 2048, misses=16, dead_run=(512, 64)), rng)
    seeds = rng.integers(0, 2**32, len(rec), dtype=np.uint64).astype(U)
    q = c.backend(pkg, ob, mat)
    got = rr.ris_compose(q, rec, seeds, 1, 1, min_t=MIN_T)
    lv = got["live"]
    smp, after = ob.light_nee(pkg.abi, c.sc.lights, rec, seeds, mat, MIN_T)
    value = rr.clamp_vec(smp[:, 8:11], rr.FLT_MAX)
    vis = np.zeros(len(rec), bool)
    vis[lv] = q.any_hit(np.ascontiguousarray(smp[lv, 0:8]))
    want = np.where(vis[:, None], value, F(0)).astype(F)
    assert dr.same_bits(got["color"][lv, 0:3], want[lv]).all() and (got["color"][:, 3] == 1.0).all()
    assert np.array_equal(got["seeds_out"][lv], rr.next_rand(after[lv])[0]) and np.array_equal(got["seeds_out"][~lv], seeds[~lv])
    assert dr.same_bits(got["color"][~lv, 0:3], rec[~lv, 12:15]).all() and (got["traced"][~lv] == 0).all()
    sel = got["reservoirs"][lv, 0, 0] != rr.NO_LIGHT
    assert sel.any() and (~sel).any() and (got["color"][lv, 0:3] > 0).any()
    assert (got["reservoirs"][lv, 0, 2][sel] == F(1).view(U)).all(), "W is exactly 1 with one candidate"
    assert np.array_equal(got["traced"][lv], sel.astype(U))
    assert np.array_equal(got["reservoirs"][lv, 0, 0][sel] & U(0xFFFF), smp.view(U)[lv, 11][sel] & U(0xFFFF))


ITEMS, PER_ITEM, CANDIDATES, DELTA = 3000, 256, 8, 1e-9


@pytest.mark.parametrize("name", ["three", "sixteen"])
def test_the_estimator_is_unbiased_against_enumeration(pkg, ob, cases, name):
    """(2) Lambertian, 3000 items, 256 independent random seeds each, K = 1, M = 8.  Truth per item: T_i = sum_k vis_k *
    clampVec(value of light k alone with lightsCount 1), from one-light oracle_light_nee calls and oracle_trace.  A single
    estimate lies in [0, R_i], R_i = lightsCount * max_k maxcomp(value_k), since term = v_sel * wsum / (M * w_sel) and
    wsum / M <= max w.  Hoeffding: |sum_i (mean_s est - T_i)| > sqrt(ln(2 / delta) / 2 * sum_i R_i^2 / S) with probability at
    most delta = 1e-9 per channel; asserted per channel, the bound from enumerated values only.
    Measured (bound, observed deviation per channel, sum T per channel) is printed; DESIGN.md "Resampled direct lighting"."""
    c = cases[name]
    rng = np.random.default_rng(2024)
    rec = c.sc.records(rng, ITEMS)
    L = len(c.sc.lights)
    q = c.backend(pkg, ob, 1)
    truth, top = np.zeros((ITEMS, 3), np.float64), np.zeros(ITEMS, np.float64)
    for k in range(L):
        smp, _ = ob.light_nee(pkg.abi, dr.one_light(pkg.abi, c.sc.lights, k), rec, np.zeros(ITEMS, U), 1, MIN_T)
        v = rr.clamp_vec(smp[:, 8:11], rr.FLT_MAX)
        vis = q.any_hit(np.ascontiguousarray(smp[:, 0:8]))
        truth += np.where(vis[:, None], v, 0).astype(np.float64)
        top = np.maximum(top, v.max(axis=1).astype(np.float64))
    R = L * top
    bound = math.sqrt(math.log(2.0 / DELTA) / 2.0 * float((R * R).sum()) / PER_ITEM)
    big = np.repeat(rec, PER_ITEM, axis=0)
    seeds = rng.integers(0, 2**32, len(big), dtype=np.uint64).astype(U)
    got = rr.ris_compose(q, big, seeds, CANDIDATES, 1, min_t=MIN_T)
    est = got["color"][:, 0:3].astype(np.float64).reshape(ITEMS, PER_ITEM, 3)
    assert (est.max(axis=1).max(axis=1) <= R * (1 + 1e-5)).all(), "a single estimate exceeds its enumerated range"
    dev = np.abs((est.mean(axis=1) - truth).sum(axis=0))
    total = truth.sum(axis=0)
    print(f"{name}: bound {bound:.4f}, deviation {dev[0]:.4f} {dev[1]:.4f} {dev[2]:.4f}, sum T {total[0]:.2f} {total[1]:.2f} {total[2]:.2f}"
          f" ({100 * bound / total.min():.2f} % of the smallest)")
    assert (dev <= bound).all(), (bound, dev)
    # what the bound can see: a missing 1 / M is off by (M - 1) * sum T, a W without wsum by a factor of the order of M
    assert bound < 0.25 * total.min(), "the bound is too loose to see a missing 1 / M or a wrong W"


# ---- the host pass -------------------------------------------------------------------------------------------------------
def test_bdpt_render_parses_and_refuses_ris_options():
    """(4) the switches that go with --ris M without it, M and K outside their ranges, a clamp that is not positive, --ris with
    --gpus / --world or with the passes it replaces exit with status 2 and a message, before any GPU is touched; --area-lights
    is read by the pass and so not refused; the usage names the options and the pass has its reference-style name"""
    import subprocess
    host = os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "host")
    names = open(os.path.join(host, "ReferenceNames.h")).read()
    assert "using bdpt::ResampledDirectPass;" in names
    head = open(os.path.join(host, "Passes.h")).read()
    for setter in ("setCandidates", "setSamples", "setMaterial", "setAreaLights", "setHints", "setClamp"):
        assert f"void {setter}(" in head.split("class ResampledDirectPass")[1].split("};")[0], setter
    render = os.path.join(host, "bdpt_render")
    if not os.path.exists(render):
        pytest.skip("host/bdpt_render not built")
    goes, needs, only = "go with --ris M", "--ris M needs M in 1 .. 32", "resampled direct lighting pass and the accumulation pass only"
    for args, text in ((["--ris-hints"], goes), (["--ris-ggx"], goes), (["--ris-samples", "2"], goes), (["--ris-clamp", "1"], goes),
                       (["--ris", "0"], needs), (["--ris", "33"], needs), (["--ris", "4", "--ris-samples", "0"], needs),
                       (["--ris", "4", "--ris-samples", "65"], needs), (["--ris", "4", "--ris-clamp", "0"], needs),
                       (["--ris", "4", "--ris-clamp", "-1"], needs), (["--ris", "4", "--gpus", "1"], needs),
                       (["--ris", "4", "--world", "2", "--rank", "0"], needs), (["--ris", "4", "--ao", "4"], only),
                       (["--ris", "4", "--gi"], only), (["--ris", "4", "--area-lights", "--denoise"], only),
                       (["--ris", "4", "--no-motion"], only)):
        r = subprocess.run([render] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and text in r.stderr, (args, r.stderr)
    u = subprocess.run([render, "--help"], capture_output=True, text=True, timeout=60)
    assert "--ris M [--ris-samples K] [--ris-ggx] [--ris-hints] [--ris-clamp C]" in u.stderr
