"""CPU checks of diffuse GI (bdpt_gi_query, bdpt_gi_execute): the ctypes structures against include/bdpt.h, the Python binding
against a fake library, the CPU yardstick of tests/gi_reference.py against a float64 reading of the reference's two shader
files, its direction restatement against oracle_bsdf, its draw counts, and the host pass under its reference name."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gi_reference as gr
from binding_fakes import ROOT, FakeGpuTensor, RecordingLib, context_without_device, desc_fields, header_layout
from edge_rays import F64_MAX_LEFT_OUT

F, U = np.float32, np.uint32
STRUCTS = {
    "bdpt_gi_desc": ("GiDesc", ["num", "flags", "numDevice", "shadeFlags", "minT", "viewPos", "reserved", "surfaces", "seeds", "alive", "color",
                                "hits", "status", "seedsOut"]),
    "bdpt_gi_params": ("GiParams", ["frameCount", "minT", "flags", "reserved"]),
}
CONSTANTS = ["BDPT_GI_INDIRECT", "BDPT_GI_UNIFORM", "BDPT_GI_SHADE_FROM_VIEW", "BDPT_GI_STATUS_DIRECT_OCCLUDED", "BDPT_GI_STATUS_BOUNCE_HIT",
             "BDPT_GI_STATUS_BOUNCE_OCCLUDED"]


def test_gi_structs_match_the_header(pkg):
    a = pkg.abi
    lay = header_layout({c: f for c, (_, f) in STRUCTS.items()}, {k: [k] for k in CONSTANTS})
    for cname, (pyname, fields) in STRUCTS.items():
        cls = getattr(a, pyname)
        assert int(lay[cname]) == C.sizeof(cls), cname
        assert [n for n, _ in cls._fields_] == fields, cname
        for name in fields:
            assert int(lay[f"{cname}.{name}"]) == getattr(cls, name).offset, (cname, name)
    assert C.sizeof(a.GiParams) == 16 and C.sizeof(a.GiDesc) == 96
    assert [int(lay[k]) for k in CONSTANTS] == [a.GI_INDIRECT, a.GI_UNIFORM, a.GI_SHADE_FROM_VIEW, a.GI_STATUS_DIRECT_OCCLUDED,
                                                a.GI_STATUS_BOUNCE_HIT, a.GI_STATUS_BOUNCE_OCCLUDED] == [1, 2, 4, 1, 2, 4]
    assert (gr.INDIRECT, gr.UNIFORM, gr.FROM_VIEW, gr.DIRECT_OCCLUDED, gr.BOUNCE_HIT, gr.BOUNCE_OCCLUDED) == (1, 2, 4, 1, 2, 4)


def test_the_entry_points_are_declared_exported_and_bound(pkg):
    a = pkg.abi
    src = open(os.path.join(ROOT, "include", "bdpt.h")).read()
    assert re.search(r"int\s+bdpt_gi_query\(bdpt_ctx\*\s*\w+,\s*const bdpt_gi_desc\*\s*\w+,\s*void\*\s*\w+\);", src)
    assert re.search(r"int\s+bdpt_gi_execute\(bdpt_ctx\*\s*\w+,\s*const bdpt_gi_params\*\s*\w+,\s*const bdpt_gbuffer\*\s*\w+,\s*float\*\s*\w+,"
                     r"\s*void\*\s*\w+\);", src)
    section = src[src.index("---- Diffuse GI"):src.index("int bdpt_gi_query(")]
    for text in ("simpleDiffuseGI.rt.hlsl", "SimpleDiffuseGIPass.cpp", "Record contract", "exactly +0", "1.0f / (2.0f * kPi)", "gCamera.posW",
                 "mDoDirectShadows"):
        assert text in section, text
    assert a.PROTOTYPES["bdpt_gi_query"] == (C.c_int, [C.c_void_p, C.POINTER(a.GiDesc), C.c_void_p])
    assert a.PROTOTYPES["bdpt_gi_execute"] == (C.c_int, [C.c_void_p, C.POINTER(a.GiParams), C.POINTER(a.GBuffer), C.c_void_p, C.c_void_p])
    raw = C.CDLL(a.LIB_PATH)
    assert hasattr(raw, "bdpt_gi_query") and hasattr(raw, "bdpt_gi_execute")
    lib = pkg.load_library()
    assert lib.bdpt_gi_query.argtypes == a.PROTOTYPES["bdpt_gi_query"][1] and lib.bdpt_gi_query.restype is C.c_int
    assert lib.bdpt_gi_query(None, None, None) == -1 and lib.bdpt_gi_execute(None, None, None, None, None) == -1  # BDPT_E_INVALID


def _ctx(pkg, device=0):
    return context_without_device(pkg, RecordingLib({"bdpt_gi_query": lambda d, stream: desc_fields(d),
                                                     "bdpt_gi_execute": lambda p, gb, out, stream: (desc_fields(p), gb, out, stream)}), device)


def test_good_calls_reach_the_library(pkg):
    import torch
    ctx = _ctx(pkg)
    f32, i32, u32, u8 = torch.float32, torch.int32, torch.uint32, torch.uint8
    n = 70
    surf, seeds = FakeGpuTensor((n, 24), f32, ptr=0x10000), FakeGpuTensor((n,), u32, ptr=0x20000)
    alive, out = FakeGpuTensor((n,), u8, ptr=0x30000), FakeGpuTensor((n, 4), f32, ptr=0x40000)
    hits, status = FakeGpuTensor((n, 4), f32, ptr=0x50000), FakeGpuTensor((n,), u32, ptr=0x60000)
    sout, cnt = FakeGpuTensor((n,), i32, ptr=0x70000), FakeGpuTensor((1,), i32, ptr=0x80000)
    res = ctx.diffuse_gi(surf, seeds, view_pos=(1.0, 2.0, 3.0), min_t=0.25, alive=alive, out=out, hits=hits, status=status, seeds_out=sout, count=cnt)
    assert res is out
    c = dict(ctx._lib.calls[-1])
    assert list(c.pop("viewPos")) == [1.0, 2.0, 3.0]
    assert c == dict(num=n, flags=1 | 4, numDevice=0x80000, shadeFlags=1, minT=0.25, reserved=0, surfaces=0x10000, seeds=0x20000, alive=0x30000,
                     color=0x40000, hits=0x50000, status=0x60000, seedsOut=0x70000)
    ctx.diffuse_gi(FakeGpuTensor((n, 24), i32, ptr=0x10000), FakeGpuTensor((n,), i32, ptr=0x20000), indirect=False, cosine=False, normal_map=False,
                   out=out)
    c = ctx._lib.calls[-1]
    assert (c["flags"], c["shadeFlags"], c["minT"], list(c["viewPos"])) == (2, 0, F(1e-4), [0.0, 0.0, 0.0])
    assert [c[k] for k in ("numDevice", "alive", "hits", "status", "seedsOut")] == [None] * 5
    ctx.diffuse_gi(surf, seeds, cosine=False, out=out, seeds_out=seeds)  # in place
    assert ctx._lib.calls[-1]["seedsOut"] == ctx._lib.calls[-1]["seeds"] == 0x20000 and ctx._lib.calls[-1]["flags"] == 3
    p, gb = pkg.abi.GiParams(0x1337, 1e-4, 3, 0), pkg.abi.GBuffer()
    ctx.gi_execute(p, gb, 0x1234, "stream")
    fields, gb_seen, out_seen, st = ctx._lib.calls[-1]
    assert fields == dict(frameCount=0x1337, minT=F(1e-4), flags=3, reserved=0) and gb_seen is gb and (out_seen, st) == (0x1234, "stream")


def test_bad_arguments_are_refused_before_the_library(pkg):
    import torch
    ctx = _ctx(pkg)
    f32, i32, u32, u8 = torch.float32, torch.int32, torch.uint32, torch.uint8
    n = 64
    good = dict(surfaces=FakeGpuTensor((n, 24), f32), seeds=FakeGpuTensor((n,), u32))
    bad = [
        dict(good, view_pos=(1.0, 2.0)), dict(good, surfaces=FakeGpuTensor((n, 24), f32, index=1)), dict(good, surfaces=FakeGpuTensor((n, 20), f32)),
        dict(good, surfaces=FakeGpuTensor((n, 24), torch.float64)), dict(good, surfaces=FakeGpuTensor((n, 24), f32, contiguous=False)),
        dict(good, seeds=FakeGpuTensor((n,), f32)), dict(good, seeds=FakeGpuTensor((n - 1,), u32)), dict(good, seeds=np.zeros(n, U)),
        dict(good, alive=FakeGpuTensor((n,), torch.bool)), dict(good, alive=FakeGpuTensor((n + 1,), u8)), dict(good, alive=torch.zeros(n, dtype=u8)),
        dict(good, out=FakeGpuTensor((n,), f32)), dict(good, out=FakeGpuTensor((n, 3), f32)), dict(good, out=FakeGpuTensor((n, 4), i32)),
        dict(good, out=torch.zeros(n, 4)), dict(good, hits=FakeGpuTensor((n,), f32)), dict(good, hits=FakeGpuTensor((n, 4), u8)),
        dict(good, status=FakeGpuTensor((n,), f32)), dict(good, status=FakeGpuTensor((n - 1,), u32)),
        dict(good, seeds_out=FakeGpuTensor((n, 1), u32)), dict(good, seeds_out=FakeGpuTensor((n,), u32, contiguous=False)),
        dict(good, count=FakeGpuTensor((2,), u32)), dict(good, count=FakeGpuTensor((1,), torch.int64)), dict(good, count=torch.ones(1, dtype=i32)),
        dict(surfaces=np.zeros((n, 24), F), seeds=np.zeros(n, U), status=FakeGpuTensor((n,), u32)),  # host arrays take no output tensors
        dict(surfaces=np.zeros((n, 20), F), seeds=np.zeros(n, U)),
    ]
    for kw in bad:
        with pytest.raises(pkg.BdptError):
            ctx.diffuse_gi(**kw)
    assert ctx._lib.calls == []


def test_frame_pipeline_diffuse_gi_passes_its_settings(pkg):
    """FramePipeline.diffuse_gi hands Context.gi_execute the pass's frame counter (from 0x1337, one per call), the pipeline's
    min_t, G-buffer and stream, and the pass's two switches"""
    import torch
    seen = []

    class Ctx:
        def gi_execute(self, p, gb, out, stream):
            seen.append((desc_fields(p), gb, out.value, stream))

    pipe = pkg.FramePipeline.__new__(pkg.FramePipeline)
    pipe.ctx, pipe.min_t, pipe.gb, pipe.gi_frame, pipe.last_gi_params = Ctx(), 0.5, "gb", 0x1337, None
    pipe.channels = {pkg.GI_CHANNEL: FakeGpuTensor((2, 3, 4), torch.float32, ptr=0x5000)}
    pipe._stream_ptr = lambda: "stream"
    out = pipe.diffuse_gi()
    assert out is pipe.channels[pkg.GI_CHANNEL]
    assert seen[-1] == (dict(frameCount=0x1337, minT=0.5, flags=1, reserved=0), "gb", 0x5000, "stream")
    pipe.diffuse_gi(indirect=False, cosine=False)
    assert seen[-1][0] == dict(frameCount=0x1338, minT=0.5, flags=2, reserved=0) and pipe.gi_frame == 0x1339
    pipe.gi_frame = 0xFFFFFFFF
    pipe.diffuse_gi(cosine=False)
    assert seen[-1][0]["frameCount"] == 0xFFFFFFFF and seen[-1][0]["flags"] == 3
    pipe.diffuse_gi()
    assert seen[-1][0]["frameCount"] == 0 and pipe.last_gi_params.frameCount == 0  # the counter wraps as a uint32 does


# ---- the CPU yardstick ---------------------------------------------------------------------------------------------------
class _Room:
    def __init__(self, pkg, ob, open_top=False):
        self.lib = ob.load_oracle(pkg.abi)
        self.sc = gr.RoomScene(pkg, open_top=open_top)
        self.osc = self.lib.oracle_scene_create(C.byref(self.sc.desc))
        assert self.osc

    def oracle(self, pkg, ob, rec, seeds, flags, **kw):
        return gr.gi_oracle(ob, pkg.abi, self.lib, self.osc, self.sc.lights, rec, seeds, flags, 1e-4, **kw)

    def close(self):
        self.lib.oracle_scene_destroy(self.osc)


@pytest.fixture(scope="module")
def room(pkg, ob):
    r = _Room(pkg, ob)
    yield r
    r.close()


def test_cosine_restatement_equals_oracle_bsdf(pkg, ob, room):
    """the numpy-float32 direction restatement, cosine variant, is oracle_bsdf's direction bit for bit (the uniform variant
    differs from it only in r and z), on unit, non-unit, zero and non-finite normals"""
    rng = np.random.default_rng(7)
    n = 4096
    _, nrm = room.sc.surface_points(rng, n)
    nrm = nrm.copy()
    nrm[::7] = rng.normal(size=(len(nrm[::7]), 3)).astype(F)
    nrm[5], nrm[12], nrm[19], nrm[26] = (0, 0, 0), (F("nan"), 0, 1), (F("inf"), 0, 0), (1e-30, 1e-30, 1e-30)
    seeds = rng.integers(0, 2**32, n, dtype=np.uint64).astype(U)
    q = gr.OracleBackend(ob, pkg.abi, room.lib, room.osc, room.sc.lights, 1e-4)
    rec = gr.ar.surface_records(np.zeros((n, 3), F), nrm)
    with np.errstate(all="ignore"):
        mine, after = gr.hemisphere_direction(room.lib, seeds, nrm, False)
        assert gr.same_bits(mine, q.cosine_direction(rec, seeds)).all()
        assert np.array_equal(after, gr.ar.lcg_chain(seeds, 2)[:, -1])
        uni, after_u = gr.hemisphere_direction(room.lib, seeds, nrm, True)
    assert np.array_equal(after_u, after)
    unit = np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1) < 1e-6
    u64, _ = gr.f64_hemisphere(seeds, nrm, True)
    assert np.abs(uni[unit].astype(np.float64) - u64[unit]).max() <= 1e-4
    assert np.abs(np.linalg.norm(uni[unit].astype(np.float64), axis=1) - 1).max() <= 1e-5
    # the height of a uniform sample is its first draw
    assert np.abs((uni[unit].astype(np.float64) * nrm[unit]).sum(axis=1) - gr.rand_float(gr.lcg(seeds))[unit]).max() <= 1e-5


@pytest.mark.parametrize("flags", [0, gr.INDIRECT, gr.UNIFORM, gr.INDIRECT | gr.UNIFORM])
def test_oracle_composition_against_a_float64_reading(pkg, ob, room, flags):
    """gi_oracle against gi_f64 on 4096 surface points of the room under three lights: every colour within 1e-4 of max(1,
    largest component), but for the items left out: a ray within F64_TOL of an edge, tmin or tmax; a closest hit with a
    runner-up within tolerance; r * lightsCount within 1e-6 of an integer; an ambiguous environment texel.  At most 2 % are
    left out.  Measured (edge / runner-up / light choice / environment of 4096): flags 0: 1 / 0 / 0 / 0; INDIRECT: 3 / 1 / 0 / 0;
    UNIFORM: 1 / 0 / 0 / 0; INDIRECT | UNIFORM: 5 / 0 / 0 / 0; with the 8 x 4 map no more."""
    rng = np.random.default_rng(41)
    n = 4096
    rec, seeds = room.sc.records(rng, n)
    for view, env in ((None, None), ((0.0, 0.0, 3.0), gr.env_map_8x4())):
        fl = flags | (gr.FROM_VIEW if view else 0)
        got = room.oracle(pkg, ob, rec, seeds, fl, view_pos=view, env=env)
        ref = gr.gi_f64(room.sc, rec, seeds, fl, 1e-4, view_pos=view, env=env)
        left = np.zeros(n, bool)
        for cause, mask in ref["left_out"].items():
            left |= mask
        counts = {k: int(v.sum()) for k, v in ref["left_out"].items()}
        print(f"flags {fl}: left out {counts} of {n}")
        assert left.mean() <= F64_MAX_LEFT_OUT, counts
        assert counts["edge"] <= 8 and counts["runner_up"] <= 2 and counts["light_choice"] == 0 and counts["environment"] <= 2, counts
        c32, c64 = got["color"][:, 0:3].astype(np.float64), ref["color"]
        tol = 1e-4 * np.maximum(1.0, np.abs(c64).max(axis=1))
        bad = (np.abs(c32 - c64).max(axis=1) > tol) & ~left
        assert not bad.any(), (int(bad.sum()), np.nonzero(bad)[0][:8])
        assert (got["color"][:, 3] == 1.0).all() and np.isfinite(c32).all() and 0 < (c32.max(axis=1) > 0).mean() < 1  # lit and unlit points both
        if flags & gr.INDIRECT:
            assert 0 < (got["status"] & gr.BOUNCE_HIT != 0).mean() < 1 and (got["status"] & gr.BOUNCE_OCCLUDED).any()
            # the hit shading of the float64 reading (face normal toward the view point, the material's colour) is the oracle's
            hit = (got["status"] & gr.BOUNCE_HIT) != 0
            assert np.abs(got["rec2"][hit, 12:15] - 1.0).max() <= 1e-6


def test_draw_counts_dead_items_and_open_room(pkg, ob):
    """0, 1 and 3 draws: a dead item keeps its seed and shows its diffuse colour; direct only advances one draw; INDIRECT
    three, whatever the sampler; in the room open at the top with an environment a tenth of the bounce rays miss"""
    o = _Room(pkg, ob, open_top=True)
    rng = np.random.default_rng(3)
    rec, seeds = o.sc.records(rng, 512, misses=32)
    alive = (np.arange(len(rec)) % 5 != 0).astype(np.uint8)
    for flags in (0, gr.UNIFORM, gr.INDIRECT, gr.INDIRECT | gr.UNIFORM):
        got = o.oracle(pkg, ob, rec, seeds, flags, alive=alive, env=np.array([0.5, 0.5, 0.8, 1.0], F))
        dead = (rec.view(np.int32)[:, 23] < 0) | (alive == 0)
        assert np.array_equal(got["live"], ~dead) and dead.sum() > 32
        draws = 3 if flags & gr.INDIRECT else 1
        assert np.array_equal(got["seeds_out"][dead], seeds[dead])
        assert np.array_equal(got["seeds_out"][~dead], gr.ar.lcg_chain(seeds[~dead], draws)[:, -1])
        assert gr.same_bits(got["color"][dead, 0:3], rec[dead, 12:15]).all() and (got["status"][dead] == 0).all()
        assert (got["hits"].view(np.int32)[dead, 3] == -1).all()
        if flags & gr.INDIRECT:
            assert ((got["status"][~dead] & gr.BOUNCE_HIT) == 0).mean() >= 0.1
        else:
            assert (got["hits"].view(np.int32)[:, 3] == -1).all()
    o.close()


# ---- the host pass -------------------------------------------------------------------------------------------------------
def test_gi_pass_compiles_under_its_reference_name():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    host = os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "host")
    src = os.path.join(ROOT, "tests", "host_compile", "gi_pass_main.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + host, src],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "using namespace" not in open(src).read().split("int main")[1]


def test_bdpt_render_refuses_bad_gi_options():
    """the sub-switches without --gi, --gi with --gpus / --world / --ao, and the switches only the replaced passes read exit
    non-zero with a message, before any GPU is touched"""
    render = os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "host", "bdpt_render")
    if not os.path.exists(render):
        pytest.skip("host/bdpt_render not built")
    for args, text in ((["--gi-uniform"], "go with --gi"), (["--gi-direct-only"], "go with --gi"), (["--gi", "--gpus", "1"], "one GPU"),
                       (["--gi", "--world", "2", "--rank", "0"], "one GPU"), (["--gi", "--ao", "4"], "not together with --ao"),
                       (["--gi", "--denoise"], "not with --denoise"), (["--gi", "--area-lights"], "not with --denoise")):
        r = subprocess.run([render] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and text in r.stderr, (args, r.stderr)
    u = subprocess.run([render, "--help"], capture_output=True, text=True, timeout=60)
    assert "--gi [--gi-direct-only] [--gi-uniform]" in u.stderr
