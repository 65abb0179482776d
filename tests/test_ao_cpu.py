"""CPU checks of ambient occlusion (bdpt_ao_query, bdpt_ao_execute): the ctypes structures against include/bdpt.h, the Python
binding's argument checks against a fake library, the CPU yardstick of tests/ao_reference.py against the oracle's RNG hook,
a float64 reading of the reference's shader and analytic anchors, and the host pass under its reference name."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ao_reference as ar
from binding_fakes import ROOT, FakeGpuTensor, RecordingLib, context_without_device, desc_fields, header_layout
from edge_rays import F64_MAX_LEFT_OUT

F, U = np.float32, np.uint32
STRUCTS = {
    "bdpt_ao_desc": ("AoDesc", ["num", "samples", "numDevice", "radius", "minT", "flags", "reserved", "surfaces", "seeds", "alive", "ao",
                                "counts", "seedsOut"]),
    "bdpt_ao_params": ("AoParams", ["frameCount", "radius", "minT", "samples", "reserved"]),
}


def test_ao_structs_match_the_header(pkg):
    a = pkg.abi
    lay = header_layout({c: f for c, (_, f) in STRUCTS.items()}, {"BDPT_AO_MAX_SAMPLES": ["BDPT_AO_MAX_SAMPLES"]})
    for cname, (pyname, fields) in STRUCTS.items():
        cls = getattr(a, pyname)
        assert int(lay[cname]) == C.sizeof(cls), cname
        assert [n for n, _ in cls._fields_] == fields, cname
        for name in fields:
            assert int(lay[f"{cname}.{name}"]) == getattr(cls, name).offset, (cname, name)
    assert C.sizeof(a.AoParams) == 20 and C.sizeof(a.AoDesc) == 80
    assert int(lay["BDPT_AO_MAX_SAMPLES"]) == a.AO_MAX_SAMPLES == 64  # the reference's GUI range


def test_the_entry_points_are_declared_exported_and_bound(pkg):
    a = pkg.abi
    src = open(os.path.join(ROOT, "include", "bdpt.h")).read()
    assert re.search(r"int\s+bdpt_ao_query\(bdpt_ctx\*\s*\w+,\s*const bdpt_ao_desc\*\s*\w+,\s*void\*\s*\w+\);", src)
    assert re.search(r"int\s+bdpt_ao_execute\(bdpt_ctx\*\s*\w+,\s*const bdpt_ao_params\*\s*\w+,\s*const bdpt_gbuffer\*\s*\w+,\s*float\*\s*\w+,"
                     r"\s*void\*\s*\w+\);", src)
    section = src[src.index("---- Ambient occlusion"):src.index("int bdpt_ao_query(")]
    assert "aoTracing.rt.hlsl:74-122" in section and "AmbientOcclusionPass.cpp:76-96" in section and "Record contract" in section
    assert a.PROTOTYPES["bdpt_ao_query"] == (C.c_int, [C.c_void_p, C.POINTER(a.AoDesc), C.c_void_p])
    assert a.PROTOTYPES["bdpt_ao_execute"] == (C.c_int, [C.c_void_p, C.POINTER(a.AoParams), C.POINTER(a.GBuffer), C.c_void_p, C.c_void_p])
    raw = C.CDLL(a.LIB_PATH)
    assert hasattr(raw, "bdpt_ao_query") and hasattr(raw, "bdpt_ao_execute")
    lib = pkg.load_library()
    assert lib.bdpt_ao_query.argtypes == a.PROTOTYPES["bdpt_ao_query"][1] and lib.bdpt_ao_query.restype is C.c_int
    assert lib.bdpt_ao_query(None, None, None) == -1 and lib.bdpt_ao_execute(None, None, None, None, None) == -1  # BDPT_E_INVALID


def _ctx(pkg, device=0):
    return context_without_device(pkg, RecordingLib({"bdpt_ao_query": lambda d, stream: desc_fields(d),
                                                     "bdpt_ao_execute": lambda p, gb, out, stream: (desc_fields(p), gb, out, stream)}), device)


def test_good_calls_reach_the_library(pkg):
    import torch
    ctx = _ctx(pkg)
    f32, i32, u32, u8 = torch.float32, torch.int32, torch.uint32, torch.uint8
    n = 70
    surf, seeds = FakeGpuTensor((n, 24), f32, ptr=0x10000), FakeGpuTensor((n,), u32, ptr=0x20000)
    alive, out = FakeGpuTensor((n,), u8, ptr=0x30000), FakeGpuTensor((n,), f32, ptr=0x40000)
    counts, sout, cnt = FakeGpuTensor((n,), u32, ptr=0x50000), FakeGpuTensor((n,), i32, ptr=0x60000), FakeGpuTensor((1,), i32, ptr=0x70000)
    res = ctx.ambient_occlusion(surf, seeds, 7, 0.5, min_t=0.25, alive=alive, out=out, counts=counts, seeds_out=sout, count=cnt)
    assert res is out
    assert ctx._lib.calls[-1] == dict(num=n, samples=7, numDevice=0x70000, radius=0.5, minT=0.25, flags=0, reserved=0, surfaces=0x10000,
                                      seeds=0x20000, alive=0x30000, ao=0x40000, counts=0x50000, seedsOut=0x60000)
    ctx.ambient_occlusion(FakeGpuTensor((n, 24), i32, ptr=0x10000), FakeGpuTensor((n,), i32, ptr=0x20000), 1, float("inf"), out=out)
    c = ctx._lib.calls[-1]
    assert (c["samples"], c["radius"], c["minT"]) == (1, float("inf"), F(1e-4))
    assert [c[k] for k in ("numDevice", "alive", "counts", "seedsOut")] == [None] * 4
    ctx.ambient_occlusion(surf, seeds, 64, 1.0, out=out, seeds_out=seeds)  # in place
    assert ctx._lib.calls[-1]["seedsOut"] == ctx._lib.calls[-1]["seeds"] == 0x20000 and ctx._lib.calls[-1]["samples"] == 64
    # the pass: the structures go through as they are
    p, gb = pkg.abi.AoParams(3, 0.5, 1e-4, 8, 0), pkg.abi.GBuffer()
    ctx.ao_execute(p, gb, 0x1234, "stream")
    fields, gb_seen, out_seen, st = ctx._lib.calls[-1]
    assert fields == dict(frameCount=3, radius=0.5, minT=F(1e-4), samples=8, reserved=0) and gb_seen is gb
    assert (out_seen, st) == (0x1234, "stream")


def test_bad_arguments_are_refused_before_the_library(pkg):
    import torch
    ctx = _ctx(pkg)
    f32, i32, u32, u8 = torch.float32, torch.int32, torch.uint32, torch.uint8
    n = 64
    surf, seeds = FakeGpuTensor((n, 24), f32), FakeGpuTensor((n,), u32)
    good = dict(surfaces=surf, seeds=seeds, samples=4, radius=1.0)
    bad = [
        dict(good, samples=0), dict(good, samples=65), dict(good, samples=-1), dict(good, samples=2.0), dict(good, samples=True),
        dict(good, samples=None),
        dict(good, surfaces=FakeGpuTensor((n, 24), f32, index=1)),                    # another GPU
        dict(good, surfaces=FakeGpuTensor((n, 24), torch.float64)),                   # dtype
        dict(good, surfaces=FakeGpuTensor((n, 20), f32)),                             # record width
        dict(good, surfaces=FakeGpuTensor((n * 24,), f32)),                           # rank
        dict(good, surfaces=FakeGpuTensor((n, 24), f32, contiguous=False)),           # strides
        dict(good, seeds=FakeGpuTensor((n,), f32)),                                   # seeds dtype
        dict(good, seeds=FakeGpuTensor((n - 1,), u32)),                               # seeds length
        dict(good, seeds=np.zeros(n, U)),                                             # one on the host, one on the GPU
        dict(good, alive=FakeGpuTensor((n,), torch.bool)),                            # alive dtype
        dict(good, alive=FakeGpuTensor((n + 1,), u8)),                                # alive length
        dict(good, alive=FakeGpuTensor((n,), u8, index=1)),
        dict(good, alive=torch.zeros(n, dtype=u8)),                                   # alive on the host
        dict(good, out=FakeGpuTensor((n, 1), f32)),                                   # out rank
        dict(good, out=FakeGpuTensor((n,), i32)),                                     # out dtype
        dict(good, out=torch.zeros(n)),                                               # out on the host
        dict(good, counts=FakeGpuTensor((n,), f32)),                                  # counts dtype
        dict(good, counts=FakeGpuTensor((n - 1,), u32)),                              # counts length
        dict(good, seeds_out=FakeGpuTensor((n, 1), u32)),                             # seeds_out rank
        dict(good, seeds_out=FakeGpuTensor((n,), u32, contiguous=False)),
        dict(good, count=FakeGpuTensor((2,), u32)),                                   # count size
        dict(good, count=FakeGpuTensor((1,), torch.int64)),                           # count dtype
        dict(good, count=torch.ones(1, dtype=i32)),                                   # count on the host
        # host arrays take no output tensors
        dict(surfaces=np.zeros((n, 24), F), seeds=np.zeros(n, U), samples=4, radius=1.0, counts=FakeGpuTensor((n,), u32)),
        dict(surfaces=np.zeros((n, 20), F), seeds=np.zeros(n, U), samples=4, radius=1.0),
    ]
    for kw in bad:
        with pytest.raises(pkg.BdptError):
            ctx.ambient_occlusion(**kw)
    assert ctx._lib.calls == []


def test_frame_pipeline_ambient_occlusion_passes_its_settings(pkg):
    """FramePipeline.ambient_occlusion hands Context.ao_execute the pass's frame counter (from 0, one per call), the
    pipeline's min_t, G-buffer and stream, and the host's default radius"""
    import torch
    seen = []

    class Ctx:
        def ao_execute(self, p, gb, out, stream):
            seen.append((desc_fields(p), gb, out.value, stream))

    pos = np.array([[0, 0, 0], [40, 0, 0], [0, 20, 0], [0, 0, 40]], F)

    class SceneStub:
        desc = pkg.abi.SceneDesc()

    SceneStub.desc.numVertices = 4
    SceneStub.desc.positions = pos.ctypes.data_as(C.POINTER(C.c_float))
    pipe = pkg.FramePipeline.__new__(pkg.FramePipeline)
    pipe.ctx, pipe.min_t, pipe.scene, pipe.gb, pipe.ao_frame, pipe.last_ao_params = Ctx(), 0.5, SceneStub, "gb", 0, None
    pipe._ao_radius = None
    pipe.channels = {pkg.AO_CHANNEL: FakeGpuTensor((2, 3, 4), torch.float32, ptr=0x5000)}
    pipe._stream_ptr = lambda: "stream"
    out = pipe.ambient_occlusion(samples=8)
    assert out is pipe.channels[pkg.AO_CHANNEL]
    # the scene radius: half the length of the half extent (20, 10, 20) = 15; the default max(0.1, 15 * 0.05) in fp32
    want = float(F(15.0) * F(0.05))
    assert pkg.ao_default_radius(SceneStub.desc) == want
    assert seen[-1] == (dict(frameCount=0, radius=F(want), minT=0.5, samples=8, reserved=0), "gb", 0x5000, "stream")
    pipe.ambient_occlusion(samples=1, radius=0.25)
    assert seen[-1][0] == dict(frameCount=1, radius=0.25, minT=0.5, samples=1, reserved=0) and pipe.ao_frame == 2
    for s in (0, 65, 1.5, True):
        with pytest.raises(pkg.BdptError):
            pipe.ambient_occlusion(samples=s)
    assert len(seen) == 2 and pipe.ao_frame == 2
    tiny = np.array([[0, 0, 0], [0.5, 0.5, 0.5]], F)
    SceneStub.desc.numVertices, SceneStub.desc.positions = 2, tiny.ctypes.data_as(C.POINTER(C.c_float))
    assert pkg.ao_default_radius(SceneStub.desc) == float(F(0.1))  # the floor of the default


# ---- the CPU yardstick -----------------------------------------------------------------------------------------------
def test_numpy_lcg_is_the_oracles_state_chain(pkg, ob):
    """the states ao_oracle walks are nextRand's: against oracle_rng's chain, draws = 2 * S for the largest S"""
    lib = ob.load_oracle(pkg.abi)
    rng = np.random.default_rng(5)
    n, draws = 257, 2 * 64
    v0, v1 = rng.integers(0, 2**32, n, dtype=np.uint64).astype(U), rng.integers(0, 2**32, n, dtype=np.uint64).astype(U)
    st, fl = np.zeros((n, draws), U), np.zeros((n, draws), F)
    lib.oracle_rng(v0.ctypes.data, v1.ctypes.data, n, draws, st.ctypes.data, fl.ctypes.data)
    assert np.array_equal(ar.lcg_chain(st[:, 0], draws - 1), st[:, 1:])
    for s in (0, 1, 0xFFFFFFFF, 0x80000000):  # the wrap-around
        assert int(ar.lcg(np.array([s], U))[0]) == (1664525 * s + 1013904223) % 2**32
    # and the floats the float64 reading derives from them are the oracle's
    assert np.array_equal(((st & U(0x00FFFFFF)).astype(np.float64) / 16777216.0).astype(F).view(U), fl.view(U))


class _Room:
    def __init__(self, pkg, ob, quads):
        self.lib = ob.load_oracle(pkg.abi)
        self.sc = ar.QuadScene(pkg, quads)
        self.osc = self.lib.oracle_scene_create(C.byref(self.sc.desc))
        assert self.osc

    def close(self):
        self.lib.oracle_scene_destroy(self.osc)


@pytest.fixture(scope="module")
def room(pkg, ob):
    r = _Room(pkg, ob, ar.room_quads())
    yield r
    r.close()


def test_oracle_composition_against_a_float64_reading(room):
    """Directions to 1e-4 (DESIGN section 2's tolerance for float64 readings); per-ray visibility equal for every ray not left
    out, with the any-hit rule only; at most F64_MAX_LEFT_OUT left out.  Measured on this scene (4096 points x 8 samples,
    radius 0.05 / 0.25 / 10 extents): 0.000 % / 0.018 % / 0.049 % left out."""
    rng = np.random.default_rng(11)
    n, S, min_t = 4096, 8, 1e-4
    pos, nrm = room.sc.surface_points(rng, n)
    seeds = rng.integers(0, 2**32, n, dtype=np.uint64).astype(U)
    rec = ar.surface_records(pos, nrm)
    dirs64 = ar.f64_directions(seeds, nrm, S)
    for frac in (0.05, 0.25, 10.0):
        radius = F(frac * room.sc.ext)
        got = ar.ao_oracle(room.lib, room.osc, rec, seeds, S, radius, min_t)
        assert np.abs(got["dirs"].astype(np.float64) - dirs64).max() <= 1e-4
        occ, left = ar.f64_any_hit(room.sc.pos, room.sc.tri, np.repeat(pos, S, axis=0), got["dirs"].reshape(-1, 3), float(F(min_t)), float(radius))
        share = left.mean()
        print(f"radius {frac} extents: {100 * share:.3f} % of {n * S} rays left out, {100 * occ.mean():.1f} % occluded")
        assert share <= F64_MAX_LEFT_OUT
        keep = ~left
        assert np.array_equal(got["vis"].reshape(-1)[keep], ~occ[keep]), int((got["vis"].reshape(-1)[keep] == occ[keep]).sum())
        assert 0 < occ.mean() < 1
        # count, division and the final state follow from the per-ray answers
        assert np.array_equal(got["counts"], got["vis"].sum(axis=1).astype(U))
        assert np.array_equal(got["ao"].view(U), (got["counts"].astype(F) / F(S)).view(U))
        assert np.array_equal(got["seeds_out"], ar.lcg_chain(seeds, 2 * S)[:, -1])


def test_analytic_anchors(pkg, ob):
    rng = np.random.default_rng(3)
    # a point on a lone floor quad sees nothing
    floor = _Room(pkg, ob, ar.floor_quads())
    n = 64
    pos = np.stack([rng.uniform(-0.9, 0.9, n), np.zeros(n), rng.uniform(-0.9, 0.9, n)], axis=1).astype(F)
    up = np.tile(np.array([[0, 1, 0]], F), (n, 1))
    seeds = rng.integers(0, 2**32, n, dtype=np.uint64).astype(U)
    got = ar.ao_oracle(floor.lib, floor.osc, ar.surface_records(pos, up), seeds, 16, 100.0, 1e-4)
    assert (got["ao"] == 1.0).all() and (got["counts"] == 16).all()
    floor.close()
    # the centre of the closed room's floor, radius above the room's size: every ray is occluded
    closed = _Room(pkg, ob, ar.room_quads(closed=True, blocks=False))
    centre = np.tile(np.array([[0, -1, 0]], F), (n, 1))
    got = ar.ao_oracle(closed.lib, closed.osc, ar.surface_records(centre, up), seeds, 16, 10.0, 1e-4)
    assert (got["ao"] == 0.0).all() and (got["counts"] == 0).all()
    # ... and with the radius at or below minT every ray misses
    for radius in (1e-4, 0.0, float("nan")):
        assert (ar.ao_oracle(closed.lib, closed.osc, ar.surface_records(centre, up), seeds, 4, radius, 1e-4)["ao"] == 1.0).all()
    # a dead item: 1.0 and its seed unchanged, beside live ones
    prim = np.where(np.arange(n) % 3 == 0, -1, 5).astype(np.int32)
    alive = (np.arange(n) % 5 != 0).astype(np.uint8)
    got = ar.ao_oracle(closed.lib, closed.osc, ar.surface_records(centre, up, prim), seeds, 4, 10.0, 1e-4, alive=alive)
    dead = (prim < 0) | (alive == 0)
    assert np.array_equal(got["live"], ~dead)
    assert (got["ao"][dead] == 1.0).all() and (got["counts"][dead] == 4).all() and np.array_equal(got["seeds_out"][dead], seeds[dead])
    assert (got["ao"][~dead] == 0.0).all() and np.array_equal(got["seeds_out"][~dead], ar.lcg_chain(seeds, 8)[~dead, -1])
    closed.close()


# ---- the host pass ---------------------------------------------------------------------------------------------------
def test_ao_pass_compiles_under_its_reference_name():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    host = os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "host")
    src = os.path.join(ROOT, "tests", "host_compile", "ao_pass_main.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + host, src],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "using namespace" not in open(src).read().split("int main")[1]


def test_bdpt_render_refuses_bad_ao_options():
    """--ao N outside 1 .. 64, a radius that is not > 0, --ao-radius without --ao, and the switches only the replaced passes
    read exit non-zero with a message, before any GPU is touched"""
    render = os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "host", "bdpt_render")
    if not os.path.exists(render):
        pytest.skip("host/bdpt_render not built")
    for args, text in ((["--ao", "0"], "--ao N needs"), (["--ao", "65"], "--ao N needs"), (["--ao", "-2"], "--ao N needs"),
                       (["--ao", "4", "--ao-radius", "0"], "R > 0"), (["--ao", "4", "--ao-radius", "-1"], "R > 0"),
                       (["--ao", "4", "--ao-radius", "nan"], "R > 0"), (["--ao", "4", "--gpus", "1"], "one GPU"),
                       (["--ao-radius", "2"], "goes with --ao"), (["--ao", "4", "--denoise"], "not with --denoise"),
                       (["--ao", "4", "--area-lights"], "not with --denoise")):
        r = subprocess.run([render] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and text in r.stderr, (args, r.stderr)
    u = subprocess.run([render, "--help"], capture_output=True, text=True, timeout=60)
    assert "--ao N [--ao-radius R]" in u.stderr
