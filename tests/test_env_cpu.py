"""CPU checks of environment lighting (bdpt_env_prepare, bdpt_env_query, bdpt_sky_query, bdpt_sky_execute and the host twins
bdpt_host_env_table / _sample / _eval): the ctypes structures against include/bdpt.h, the Python binding's argument checks
against a fake library, the host table against the exact-integer restatement of tests/env_numpy.py, the table search against
numpy's searchsorted, a float64 reading of the sampler, normalisation, the sample -> eval round trip, a binomial check on the
sun map, and the stand-alone sanitizer program."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import env_numpy as en
from binding_fakes import ROOT, FakeGpuTensor, RecordingLib, context_without_device, desc_fields, header_layout

F, U, D = np.float32, np.uint32, np.float64
STRUCTS = {
    "bdpt_env_info": ("EnvInfo", ["width", "height", "total", "max", "rowScanChunk", "marginalChunk", "reserved", "tableBytes", "cdf", "rowCdf"]),
    "bdpt_env_sample": ("EnvSample", ["ray", "radiance", "pdf", "value", "texel", "status", "reserved"]),
    "bdpt_env_eval": ("EnvEval", ["radiance", "pdf", "texel", "reserved"]),
    "bdpt_env_host_sample": ("EnvHostSample", ["dir", "pdf", "radiance", "texel"]),
    "bdpt_env_desc": ("EnvDesc", ["mode", "num", "numDevice", "matIndex", "flags", "minT", "reserved", "surfaces", "seeds", "seedsOut", "samples",
                                  "dirs", "evals", "compactRays", "compactItems", "compactCount"]),
    "bdpt_sky_desc": ("SkyDesc", ["num", "samples", "numDevice", "clampUpper", "minT", "flags", "reserved", "surfaces", "seeds", "alive", "color",
                                  "counts", "seedsOut"]),
    "bdpt_sky_params": ("SkyParams", ["frameCount", "clampUpper", "minT", "samples", "reserved"]),
}
ENTRY_POINTS = ["bdpt_env_prepare", "bdpt_get_env_info", "bdpt_env_query", "bdpt_sky_query", "bdpt_sky_execute", "bdpt_host_env_table",
                "bdpt_host_env_sample", "bdpt_host_env_eval", "bdpt_test_env_table", "bdpt_test_host_env_search"]


def test_env_structs_match_the_header(pkg):
    a = pkg.abi
    consts = {"C": ["BDPT_ENV_MAX_DIM", "BDPT_ENV_SAMPLE", "BDPT_ENV_EVAL", "BDPT_ENV_STATUS_NONZERO", "BDPT_SKY_MAX_SAMPLES"]}
    lay = header_layout({c: f for c, (_, f) in STRUCTS.items()}, consts)
    for cname, (pyname, fields) in STRUCTS.items():
        cls = getattr(a, pyname)
        assert int(lay[cname]) == C.sizeof(cls), cname
        assert [n for n, _ in cls._fields_] == fields, cname
        for name in fields:
            assert int(lay[f"{cname}.{name}"]) == getattr(cls, name).offset, (cname, name)
    assert [C.sizeof(getattr(a, n)) for n in ("EnvInfo", "EnvSample", "EnvEval", "EnvHostSample", "EnvDesc", "SkyDesc", "SkyParams")] == \
        [56, 80, 32, 32, 104, 80, 20]
    assert [int(v) for v in lay["C"].split()] == [a.ENV_MAX_DIM, a.ENV_SAMPLE, a.ENV_EVAL, a.ENV_STATUS_NONZERO, a.SKY_MAX_SAMPLES] == \
        [16384, 0, 1, 1, 64]
    assert en.SAMPLE_DT.itemsize == C.sizeof(a.EnvHostSample) and en.EVAL_DT.itemsize == C.sizeof(a.EnvEval)
    # the scan chunk sizes the binding states are the header's (csrc/env_light.h)
    src = open(os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "csrc", "env_light.h")).read()
    assert int(re.search(r"kEnvRowScanChunk = (\d+);", src).group(1)) == a.ENV_ROW_SCAN_CHUNK
    assert int(re.search(r"kEnvMarginalChunk = (\d+);", src).group(1)) == a.ENV_MARGINAL_CHUNK


def test_the_entry_points_are_declared_exported_and_bound(pkg):
    a = pkg.abi
    src = open(os.path.join(ROOT, "include", "bdpt.h")).read()
    assert re.search(r"int\s+bdpt_env_prepare\(bdpt_ctx\*\s*\w+,\s*void\*\s*\w+\);", src)
    assert re.search(r"int\s+bdpt_env_query\(bdpt_ctx\*\s*\w+,\s*const bdpt_env_desc\*\s*\w+,\s*void\*\s*\w+\);", src)
    assert re.search(r"int\s+bdpt_sky_query\(bdpt_ctx\*\s*\w+,\s*const bdpt_sky_desc\*\s*\w+,\s*void\*\s*\w+\);", src)
    assert re.search(r"int\s+bdpt_sky_execute\(bdpt_ctx\*\s*\w+,\s*const bdpt_sky_params\*\s*\w+,\s*const bdpt_gbuffer\*\s*\w+,\s*float\*\s*\w+,"
                     r"\s*void\*\s*\w+\);", src)
    section = src[src.index("---- Environment lighting"):src.index("int bdpt_env_prepare(")]
    for text in ("65535.0", "rowCdf", "exactly four draws", "Build definition", "Record contract", "bit for bit", "2^-24"):
        assert text in section, text
    assert a.PROTOTYPES["bdpt_env_query"] == (C.c_int, [C.c_void_p, C.POINTER(a.EnvDesc), C.c_void_p])
    assert a.PROTOTYPES["bdpt_sky_query"] == (C.c_int, [C.c_void_p, C.POINTER(a.SkyDesc), C.c_void_p])
    assert a.PROTOTYPES["bdpt_sky_execute"] == (C.c_int, [C.c_void_p, C.POINTER(a.SkyParams), C.POINTER(a.GBuffer), C.c_void_p, C.c_void_p])
    raw = C.CDLL(a.LIB_PATH)
    lib = pkg.load_library()
    for name in ENTRY_POINTS:
        assert re.search(r"int\s+" + name + r"\(", src) and hasattr(raw, name) and name in a.PROTOTYPES, name
        assert getattr(lib, name).argtypes == a.PROTOTYPES[name][1]
    assert lib.bdpt_env_query(None, None, None) == -1 and lib.bdpt_sky_query(None, None, None) == -1  # BDPT_E_INVALID
    assert lib.bdpt_sky_execute(None, None, None, None, None) == -1 and lib.bdpt_env_prepare(None, None) == -1
    assert lib.bdpt_get_env_info(None, None) == -1 and lib.bdpt_test_env_table(None, None, None) == -1
    # the host twins' own refusals: missing arrays, a zero size, a size past the limit
    z = np.zeros(16, F)
    assert lib.bdpt_host_env_table(None, 1, 1, None, z.ctypes.data, z.ctypes.data, None) == -1
    assert lib.bdpt_host_env_table(z.ctypes.data, 0, 1, None, z.ctypes.data, z.ctypes.data, None) == -1
    assert lib.bdpt_host_env_table(z.ctypes.data, 16385, 1, None, z.ctypes.data, z.ctypes.data, None) == -5  # BDPT_E_LIMIT
    assert lib.bdpt_host_env_sample(z.ctypes.data, 1, 16385, z.ctypes.data, z.ctypes.data, z.ctypes.data, 0, None, None) == -5
    assert lib.bdpt_host_env_eval(z.ctypes.data, 1, 1, z.ctypes.data, z.ctypes.data, None, 1, z.ctypes.data) == -1


def _ctx(pkg, device=0):
    return context_without_device(pkg, RecordingLib({
        "bdpt_env_query": lambda d, stream: desc_fields(d), "bdpt_sky_query": lambda d, stream: desc_fields(d),
        "bdpt_sky_execute": lambda p, gb, out, stream: (desc_fields(p), gb, out, stream),
        "bdpt_env_prepare": lambda stream: ("prepare", stream), "bdpt_set_environment": lambda e: ("set", desc_fields(e))}), device)


def test_good_calls_reach_the_library(pkg):
    import torch
    a = pkg.abi
    ctx = _ctx(pkg)
    f32, i32, u32, u8 = torch.float32, torch.int32, torch.uint32, torch.uint8
    n = 70
    surf, seeds = FakeGpuTensor((n, 24), f32, ptr=0x10000), FakeGpuTensor((n,), u32, ptr=0x20000)
    out, sout, cnt = FakeGpuTensor((n, 20), f32, ptr=0x30000), FakeGpuTensor((n,), i32, ptr=0x40000), FakeGpuTensor((1,), i32, ptr=0x50000)
    comp = (FakeGpuTensor((n, 8), f32, ptr=0x60000), FakeGpuTensor((n,), u32, ptr=0x70000), FakeGpuTensor((1,), u32, ptr=0x80000))
    assert ctx.env_sample(surf, seeds, mat_index=0, min_t=0.25, out=out, seeds_out=sout, compact=comp, count=cnt) is out
    assert ctx._lib.calls[-1] == dict(mode=a.ENV_SAMPLE, num=n, numDevice=0x50000, matIndex=0, flags=0, minT=0.25, reserved=0, surfaces=0x10000,
                                      seeds=0x20000, seedsOut=0x40000, samples=0x30000, dirs=None, evals=None, compactRays=0x60000,
                                      compactItems=0x70000, compactCount=0x80000)
    ctx.env_sample(surf, seeds, out=out)
    c = ctx._lib.calls[-1]
    assert (c["matIndex"], c["minT"], c["seedsOut"], c["compactRays"], c["numDevice"]) == (1, F(1e-4), None, None, None)
    dirs, ev = FakeGpuTensor((n, 4), f32, ptr=0x11000), FakeGpuTensor((n, 8), f32, ptr=0x12000)
    assert ctx.env_eval(dirs, out=ev, count=cnt) is ev
    c = ctx._lib.calls[-1]
    assert (c["mode"], c["num"], c["dirs"], c["evals"], c["numDevice"], c["surfaces"]) == (a.ENV_EVAL, n, 0x11000, 0x12000, 0x50000, None)
    col, alive, counts = FakeGpuTensor((n, 4), f32, ptr=0x13000), FakeGpuTensor((n,), u8, ptr=0x14000), FakeGpuTensor((n,), u32, ptr=0x15000)
    assert ctx.sky_lighting(surf, seeds, 7, clamp=2.5, min_t=0.5, alive=alive, out=col, counts=counts, seeds_out=seeds, count=cnt) is col
    assert ctx._lib.calls[-1] == dict(num=n, samples=7, numDevice=0x50000, clampUpper=2.5, minT=0.5, flags=0, reserved=0, surfaces=0x10000,
                                      seeds=0x20000, alive=0x14000, color=0x13000, counts=0x15000, seedsOut=0x20000)
    ctx.sky_lighting(surf, seeds, 64, out=col)
    assert ctx._lib.calls[-1]["clampUpper"] == en.FLT_MAX and ctx._lib.calls[-1]["samples"] == 64
    p, gb = a.SkyParams(3, 1.0, 1e-4, 8, 0), a.GBuffer()
    ctx.sky_execute(p, gb, 0x1234, "stream")
    fields, gb_seen, out_seen, st = ctx._lib.calls[-1]
    assert fields == dict(frameCount=3, clampUpper=1.0, minT=F(1e-4), samples=8, reserved=0) and gb_seen is gb and (out_seen, st) == (0x1234, "stream")


def test_bad_arguments_are_refused_before_the_library(pkg):
    import torch
    ctx = _ctx(pkg)
    f32, i32, u32, u8 = torch.float32, torch.int32, torch.uint32, torch.uint8
    n = 64
    surf, seeds = FakeGpuTensor((n, 24), f32), FakeGpuTensor((n,), u32)
    good = dict(surfaces=surf, seeds=seeds, samples=4)
    bad_sky = [
        dict(good, samples=0), dict(good, samples=65), dict(good, samples=-1), dict(good, samples=2.0), dict(good, samples=True),
        dict(good, samples=None), dict(good, surfaces=FakeGpuTensor((n, 24), f32, index=1)), dict(good, surfaces=FakeGpuTensor((n, 20), f32)),
        dict(good, surfaces=FakeGpuTensor((n, 24), f32, contiguous=False)), dict(good, seeds=FakeGpuTensor((n,), f32)),
        dict(good, seeds=FakeGpuTensor((n - 1,), u32)), dict(good, seeds=np.zeros(n, U)), dict(good, alive=FakeGpuTensor((n,), torch.bool)),
        dict(good, alive=FakeGpuTensor((n + 1,), u8)), dict(good, out=FakeGpuTensor((n,), f32)), dict(good, out=FakeGpuTensor((n, 4), i32)),
        dict(good, out=torch.zeros(n, 4)), dict(good, counts=FakeGpuTensor((n,), f32)), dict(good, seeds_out=FakeGpuTensor((n, 1), u32)),
        dict(good, count=FakeGpuTensor((2,), u32)), dict(good, count=torch.ones(1, dtype=i32)),
        dict(surfaces=np.zeros((n, 24), F), seeds=np.zeros(n, U), samples=4, counts=FakeGpuTensor((n,), u32)),
    ]
    for kw in bad_sky:
        with pytest.raises(pkg.BdptError):
            ctx.sky_lighting(**kw)
    good = dict(surfaces=surf, seeds=seeds)
    comp = (FakeGpuTensor((n, 8), f32), FakeGpuTensor((n,), u32), FakeGpuTensor((1,), u32))
    bad_sample = [
        dict(good, mat_index=2), dict(good, mat_index=True), dict(good, surfaces=FakeGpuTensor((n, 23), f32)), dict(good, seeds=FakeGpuTensor((n,), u8)),
        dict(good, out=FakeGpuTensor((n, 12), f32)), dict(good, seeds_out=FakeGpuTensor((n + 1,), u32)), dict(good, compact=comp[:2]),
        dict(good, compact=(comp[0], None, comp[2])), dict(good, compact=(FakeGpuTensor((n, 4), f32), comp[1], comp[2])),
        dict(good, compact=(comp[0], comp[1], FakeGpuTensor((2,), u32))), dict(good, seeds=np.zeros(n, U)),
    ]
    for kw in bad_sample:
        with pytest.raises(pkg.BdptError):
            ctx.env_sample(**kw)
    for dirs in (FakeGpuTensor((n, 3), f32), FakeGpuTensor((n, 4), torch.float64), FakeGpuTensor((n, 4), f32, index=1), np.zeros((n, 3), F)):
        with pytest.raises(pkg.BdptError):
            ctx.env_eval(dirs)
    with pytest.raises(pkg.BdptError):
        ctx.env_eval(FakeGpuTensor((n, 4), f32), out=FakeGpuTensor((n, 4), f32))
    assert ctx._lib.calls == []


def test_frame_pipeline_sky_lighting_keeps_its_counter_and_prepares_anew(pkg):
    """FramePipeline.sky_lighting hands Context.sky_execute its own frame counter (from 0, one per call), the pipeline's min_t,
    G-buffer and stream; the table is prepared on first use and again after every set_environment, not otherwise"""
    import torch
    ctx = _ctx(pkg)
    pipe = pkg.FramePipeline.__new__(pkg.FramePipeline)
    pipe.ctx, pipe.min_t, pipe.gb, pipe.sky_frame, pipe.last_sky_params = ctx, 0.5, pkg.abi.GBuffer(), 0, None
    pipe.torch, pipe.dev, pipe.H, pipe.W = torch, None, 2, 3
    pipe.channels = {pkg.SKY_CHANNEL: FakeGpuTensor((2, 3, 4), torch.float32, ptr=0x5000)}
    pipe._stream_ptr = lambda: "stream"
    ctx.set_environment(0x9000, 8, 4)
    assert ctx._lib.calls[-1][0] == "set" and ctx._lib.calls[-1][1]["envMap"] == 0x9000
    out = pipe.sky_lighting(samples=8, clamp=2.0)
    assert out is pipe.channels[pkg.SKY_CHANNEL]
    assert ctx._lib.calls[-2] == ("prepare", "stream")
    fields, gb, ptr, st = ctx._lib.calls[-1]
    assert fields == dict(frameCount=0, clampUpper=2.0, minT=0.5, samples=8, reserved=0) and gb is pipe.gb and st == "stream"
    assert ptr.value == 0x5000
    n = len(ctx._lib.calls)
    pipe.sky_lighting()
    assert len(ctx._lib.calls) == n + 1  # no second prepare
    assert ctx._lib.calls[-1][0] == dict(frameCount=1, clampUpper=en.FLT_MAX, minT=0.5, samples=1, reserved=0) and pipe.sky_frame == 2
    ctx.set_environment(0xA000, 8, 4)  # a new probe
    pipe.sky_lighting(samples=2)
    assert ctx._lib.calls[-2] == ("prepare", "stream") and ctx._lib.calls[-1][0]["frameCount"] == 2
    assert pipe.last_sky_params.samples == 2
    n = len(ctx._lib.calls)
    for s in (0, 65, 1.5, True):
        with pytest.raises(pkg.BdptError):
            pipe.sky_lighting(samples=s)
    assert len(ctx._lib.calls) == n and pipe.sky_frame == 3


# ---- the table -------------------------------------------------------------------------------------------------------
_cache = {}


def _maps(pkg):
    """{name: (map, host table, numpy table)}, made once"""
    if "maps" not in _cache:
        lib = pkg.load_library()
        a = pkg.abi
        _cache["maps"] = {name: (env, en.host_table(lib, env), en.table(env)) for name, env in en.maps(a.ENV_ROW_SCAN_CHUNK, a.ENV_MARGINAL_CHUNK).items()}
    return _cache["maps"]


def test_host_table_equals_the_exact_integer_restatement(pkg):
    """q, cdf, rowCdf, total and m of every map of the list equal numpy's, word for word"""
    a = pkg.abi
    ms = _maps(pkg)
    assert {(env.shape[1], env.shape[0]) for env, _, _ in ms.values()} >= {(1, 1), (2, 1), (1, 2), (7, 5), (64, 32), (a.ENV_ROW_SCAN_CHUNK + 1, 2),
                                                                           (2, a.ENV_MARGINAL_CHUNK + 1)}
    for name, (env, got, want) in ms.items():
        for k in ("q", "cdf", "row_cdf"):
            assert np.array_equal(got[k], want[k]), (name, k)
        assert got["total"] == want["total"] and got["m"].view(U) == want["m"].view(U), name
        assert int(want["q"].sum(dtype=np.uint64)) == want["total"]
        assert want["q"].max(initial=0) <= 65536 and want["total"] <= 2**44
        # any positive channel makes the texel reachable; none makes it unreachable
        with np.errstate(invalid="ignore"):
            lit = (env[..., :3] > 0).any(axis=-1)
        assert np.array_equal(want["q"] > 0, lit), name
        if lit.any():
            assert want["q"].max() == 65536  # the maximum's own texel
    assert ms["zero"][1]["total"] == 0 and (ms["zero"][1]["cdf"] == 0).all()
    sun = ms["sun"][2]
    assert sun["q"][en.SUN_TEXEL[1], en.SUN_TEXEL[0]] == 65536 and (sun["q"][5] == 0).all() and (sun["q"][20] == 0).all()
    assert (np.diff(sun["row_cdf"])[[4, 19]] == 0).all()  # the empty rows add nothing
    edge = ms["edge"][2]["q"].reshape(-1)
    assert list(edge > 0) == [False, True, True, True, False, True, True, True, True, False, False, True, True, True, True, True]
    sub = ms["subnormal"][2]
    assert sub["m"] < F(1.2e-38) and sub["total"] > 0


def _boundary_seeds(tab, extra=4096, seed=0):
    """states whose first two draws reach the tables' boundary values: r1 aimed at every rowCdf boundary and its neighbours;
    r2 follows from r1 (an LCG's low 24 bits are a function of its low 24 bits), so the column boundaries are met by picking,
    from a 2^20 stride of all first draws, those whose t2 is a boundary value of its row or next to one"""
    total = tab["total"]
    rng = np.random.default_rng(seed)
    r1 = [rng.integers(0, 2**24, extra), np.array([0, 1, 2**24 - 2, 2**24 - 1])]
    if total:
        b = np.unique(np.concatenate([[0], tab["row_cdf"].astype(np.int64)]))
        for off in (-2, -1, 0, 1, 2):
            t = np.clip(b + off, 0, total - 1)
            r = -((-t * 2**24) // total)  # the smallest r1 with floor(r1 total / 2^24) >= t
            r1 += [np.clip(r, 0, 2**24 - 1), np.clip(r - 1, 0, 2**24 - 1)]
        grid = np.arange(0, 2**24, 16, dtype=np.int64)
        s1 = grid.astype(U)
        r2 = (en.lcg(s1) & U(0xFFFFFF)).astype(np.int64)
        t = np.minimum((grid * total) >> 24, total - 1).astype(np.uint64)
        y = np.searchsorted(tab["row_cdf"], t, side="right")
        rt = tab["cdf"][y, -1].astype(np.int64)
        t2 = np.minimum((r2 * rt) >> 24, rt - 1)
        near = np.zeros(len(grid), bool)
        for off in (-1, 0):  # t2 == cdf[y][x] - 1 (the last value of texel x) or == cdf[y][x] (the first of the next lit one)
            flat = (tab["cdf"].astype(np.int64) + off)
            for yy in np.unique(y):
                sel = y == yy
                near[sel] |= np.isin(t2[sel], flat[yy])
        pick = np.nonzero(near)[0]
        if len(pick) > 20000:
            pick = pick[:: len(pick) // 20000 + 1]
        r1.append(grid[pick])
    r1 = np.unique(np.concatenate([np.asarray(r, np.int64) for r in r1]))
    return en.seeds_for_first_draw(r1.astype(U))


def test_search_equals_searchsorted_on_every_boundary(pkg):
    """bdpt_host_env_sample's texel equals numpy's searchsorted on the integer tables for draws at and beside every rowCdf
    boundary and the cdf boundaries; all-zero output and four draws with total == 0"""
    lib = pkg.load_library()
    for name, (env, tab, _) in _maps(pkg).items():
        H, W = env.shape[:2]
        seeds = _boundary_seeds(tab)
        d, after = en.draws(seeds)
        got, sout = en.host_sample(lib, env, tab, seeds)
        assert np.array_equal(sout, after), name  # exactly four draws
        if tab["total"] == 0:
            assert not got.view(np.uint8).any(), name
            continue
        x, y = en.search(tab, d[:, 0], d[:, 1])
        assert np.array_equal(got["texel"].astype(np.int64), y * W + x), (name, int((got["texel"] != y * W + x).sum()))
        assert (tab["q"][y, x] > 0).all(), name  # never an unlit texel
        assert np.array_equal(got["radiance"].view(U), env[y, x, :3].view(U)), name
        # coverage: every row with weight was drawn, and both sides of column boundaries were met
        rows_lit = np.nonzero(np.diff(np.concatenate([[0], tab["row_cdf"].astype(np.int64)])) > 0)[0]
        assert tab["total"] <= 2**24  # (so a 24-bit draw reaches every value of t)
        assert set(rows_lit) <= set(np.unique(y)), name
        if W > 1 and (tab["q"] > 0).sum() > H:
            assert len(np.unique(y * W + x)) >= min(int((tab["q"] > 0).sum()), 16), name


def test_search_on_a_grid_of_draws_at_every_boundary(pkg):
    """bdpt_test_host_env_search (envSearch, the sampler's search, on draws given directly) against numpy's searchsorted: for
    every lit row a first draw at the row's first and last value of t and one beyond each, and for every boundary value c
    of that row's cdf (and 0) second draws whose t2 is c - 1, c and c + 1.  Every such t and t2 is met exactly (the totals
    are below 2^24, so a 24-bit draw reaches every value), and every lit texel is returned at least once."""
    lib = pkg.load_library()
    for name, (env, tab, _) in _maps(pkg).items():
        H, W = env.shape[:2]
        total = tab["total"]
        cdf, row_cdf = np.ascontiguousarray(tab["cdf"], U), np.ascontiguousarray(tab["row_cdf"], np.uint64)
        one = np.zeros(1, F)
        if total == 0:
            assert lib.bdpt_test_host_env_search(W, H, cdf.ctypes.data, row_cdf.ctypes.data, one.ctypes.data, one.ctypes.data, 1, one.ctypes.data) == -2
            continue
        assert total <= 2**24 and int(cdf[:, -1].max()) <= 2**24
        draw_for = lambda t, n: -((-t * 2**24) // n)  # the smallest 24-bit draw r with floor(r n / 2^24) >= t
        starts = np.concatenate([[0], tab["row_cdf"].astype(np.int64)])
        r1s, r2s, want_t, want_t2, aim = [], [], [], [], []
        for y in np.nonzero(np.diff(starts) > 0)[0]:
            rt = int(cdf[y, -1])
            t2 = np.unique(np.clip(np.concatenate([[0], cdf[y].astype(np.int64)])[:, None] + np.array([-1, 0, 1])[None, :], 0, rt - 1))
            for t in np.unique(np.clip([starts[y] - 1, starts[y], starts[y] + 1, starts[y + 1] - 1, starts[y + 1]], 0, total - 1)):
                r1s.append(np.full(len(t2), draw_for(int(t), total)))
                r2s.append(draw_for(t2, rt))
                want_t.append(np.full(len(t2), t))
                want_t2.append(t2)
                aim.append(np.full(len(t2), y))
        r1, r2, want_t, want_t2, aim = (np.concatenate(a).astype(np.int64) for a in (r1s, r2s, want_t, want_t2, aim))
        assert r1.max() < 2**24 and r2.max() < 2**24
        assert np.array_equal((r1 * total) >> 24, want_t), name  # every aimed-at value of t is met
        f1, f2 = (r1.astype(D) / 16777216.0).astype(F), (r2.astype(D) / 16777216.0).astype(F)
        got = np.zeros(len(r1), U)
        assert lib.bdpt_test_host_env_search(W, H, cdf.ctypes.data, row_cdf.ctypes.data, f1.ctypes.data, f2.ctypes.data, len(r1), got.ctypes.data) == 0
        x, y = en.search(tab, r1, r2)
        own = (r2 * cdf[y, -1].astype(np.int64)) >> 24  # t2 in the row the first draw chose
        in_row = y == aim  # (a first draw one beyond the row's values lands in a neighbouring row: compared, not aimed)
        assert in_row[(want_t >= starts[aim]) & (want_t < starts[aim + 1])].all(), name  # a t inside the row finds the row
        assert np.array_equal(own[in_row], want_t2[in_row]), name  # and there every aimed-at t2 is met
        assert np.array_equal(got.astype(np.int64), y * W + x), (name, int((got != y * W + x).sum()))
        assert (tab["q"][y, x] > 0).all(), name
        assert set(np.unique(got)) == set(np.nonzero(tab["q"].reshape(-1) > 0)[0]), name  # every lit texel, and only those


PDF_MIN_SINE = 2.0 ** -8


def test_directions_and_pdf_against_a_float64_reading(pkg):
    """dir within 1e-4 (DESIGN section 2's bar for float64 readings) of (-sin(pi v) sin(2 pi u), cos(pi v), sin(pi v)
    cos(2 pi u)); pdf within 1e-4 relative of (q / total) W H / (2 pi^2 sin(pi v)) for every sample whose float64 sin(pi v)
    is above PDF_MIN_SINE = 2^-8 (include/bdpt.h "Environment lighting" states the threshold): v is an fp32 number up to 1
    with two roundings behind it, so it is off by up to 1.2e-7, sin(pi v) by pi times that, 3.7e-7, and 1e-4 of the sine is
    no less than that only from a sine of 3.7e-3 on.  At most 1 % of the samples of any map are left out."""
    lib = pkg.load_library()
    rng = np.random.default_rng(9)
    worst_left_out = 0.0
    for name, (env, tab, _) in _maps(pkg).items():
        if tab["total"] == 0:
            continue
        H, W = env.shape[:2]
        seeds = rng.integers(0, 2**32, 4096, dtype=np.uint64).astype(U)
        d, _ = en.draws(seeds)
        got, _ = en.host_sample(lib, env, tab, seeds)
        y, x = np.divmod(got["texel"].astype(np.int64), W)
        dir64, pdf64, st, _, _ = en.f64_sample(tab, W, H, x, y, d[:, 2], d[:, 3])
        assert np.abs(got["dir"].astype(D) - dir64).max() <= 1e-4, name
        ok = st > PDF_MIN_SINE
        worst_left_out = max(worst_left_out, float((~ok).mean()))
        assert (~ok).mean() <= 0.01, (name, float((~ok).mean()))
        rel = np.abs(got["pdf"][ok].astype(D) - pdf64[ok]) / pdf64[ok]
        assert (rel <= 1e-4).all(), (name, float(rel.max()))
        assert (got["pdf"][st > 0] > 0).all()
    print(f"largest share of samples left out below sin(theta) = 2^-8: {100 * worst_left_out:.3f} %")


def test_normalisation(pkg):
    """sum q / total == 1 exactly (integers), and the pdf bdpt_host_env_eval returns integrates to 1 over the sphere within
    1e-4: a midpoint rule with every texel row split so that the rule's own error, (pi / (2 H K))^2 / 6, is below 1e-5"""
    lib = pkg.load_library()
    for name, (env, tab, _) in _maps(pkg).items():
        assert int(tab["q"].sum(dtype=np.uint64)) == tab["total"], name
        if tab["total"] == 0:
            continue
        H, W = env.shape[:2]
        K = max(1, math.ceil(420 / H))
        assert (math.pi / (2 * H * K)) ** 2 / 6 < 1e-5
        v = (np.arange(H * K) + 0.5) / (H * K)
        u = (np.arange(W) + 0.5) / W
        vv, uu = np.meshgrid(v, u, indexing="ij")
        st, ct = np.sin(np.pi * vv), np.cos(np.pi * vv)
        dirs = np.stack([-st * np.sin(2 * np.pi * uu), ct, st * np.cos(2 * np.pi * uu)], axis=-1).reshape(-1, 3)
        ev = en.host_eval(lib, env, tab, dirs.astype(F))
        ty, tx = np.repeat(np.arange(H), K)[:, None].repeat(W, axis=1), np.arange(W)[None, :].repeat(H * K, axis=0)
        assert np.array_equal(ev["texel"].astype(np.int64), (ty * W + tx).reshape(-1)), name  # cell centres: far from every border
        theta0, theta1 = np.pi * np.arange(H * K) / (H * K), np.pi * (np.arange(H * K) + 1) / (H * K)
        omega = ((2 * np.pi / W) * (np.cos(theta0) - np.cos(theta1)))[:, None].repeat(W, axis=1).reshape(-1)
        integral = float((ev["pdf"].astype(D) * omega).sum())
        assert abs(integral - 1.0) <= 1e-4, (name, integral)


def _round_trip(pkg, name):
    lib = pkg.load_library()
    env, tab, _ = _maps(pkg)[name]
    H, W = env.shape[:2]
    rng = np.random.default_rng(13)
    seeds = rng.integers(0, 2**32, 8192, dtype=np.uint64).astype(U)
    d, _ = en.draws(seeds)
    got, _ = en.host_sample(lib, env, tab, seeds)
    y, x = np.divmod(got["texel"].astype(np.int64), W)
    _, _, st, uw, vh = en.f64_sample(tab, W, H, x, y, d[:, 2], d[:, 3])
    keep = en.border_distance(uw, vh) > 2.0 ** -10
    back = en.host_eval(lib, env, tab, got["dir"])
    return got, back, keep, st


ROUND_TRIP_MAPS = ["1x1", "2x1", "1x2", "7x5", "sun", "edge", "subnormal", "wide", "tall", "wide2"]


@pytest.mark.parametrize("name", ROUND_TRIP_MAPS)
def test_round_trip_returns_the_sampled_texel(pkg, name):
    """bdpt_host_env_eval of a sampled direction returns the sampled texel and its radiance for every sample whose float64
    (u W, v H) lies farther than 2^-10 from a texel border; at most 1 % of the samples are left out"""
    got, back, keep, _ = _round_trip(pkg, name)
    assert (~keep).mean() <= 0.01, float((~keep).mean())
    assert np.array_equal(back["texel"][keep], got["texel"][keep]), int((back["texel"][keep] != got["texel"][keep]).sum())
    assert np.array_equal(back["radiance"][keep].view(U), got["radiance"][keep].view(U))


@pytest.mark.parametrize("name", ROUND_TRIP_MAPS)
def test_round_trip_pdfs_agree(pkg, name):
    """where the texel agrees, the sampler's pdf and bdpt_host_env_eval's agree within 1e-4 relative"""
    got, back, keep, st = _round_trip(pkg, name)
    same = keep & (back["texel"] == got["texel"]) & (got["pdf"] > 0)
    a, b = got["pdf"][same].astype(D), back["pdf"][same].astype(D)
    rel = np.abs(a - b) / a
    worst = int(np.argmax(rel))
    print(f"{name}: {int((rel > 1e-4).sum())} of {same.sum()} beyond 1e-4, worst {rel.max():.3e} at sin(theta) = {st[same][worst]:.3e}")
    assert (rel <= 1e-4).all(), (name, float(rel.max()), int((rel > 1e-4).sum()))


def test_sun_map_share_of_draws(pkg):
    """4096 samples of the 64 x 32 sun map: the sun texel's share lies within 5 binomial standard deviations of q / total"""
    lib = pkg.load_library()
    env, tab, _ = _maps(pkg)["sun"]
    n = 4096
    seeds = np.random.default_rng(31).integers(0, 2**32, n, dtype=np.uint64).astype(U)
    got, _ = en.host_sample(lib, env, tab, seeds)
    sun = en.SUN_TEXEL[1] * env.shape[1] + en.SUN_TEXEL[0]
    p = 65536 / tab["total"]
    assert tab["q"][en.SUN_TEXEL[1], en.SUN_TEXEL[0]] == 65536 and 0.5 < p < 1
    hits = int((got["texel"] == sun).sum())
    sd = math.sqrt(n * p * (1 - p))
    print(f"sun texel: {hits} of {n} draws, expected {n * p:.1f} +- {sd:.1f}")
    assert abs(hits - n * p) <= 5 * sd
    # the sky texels share the rest: each has q = 1
    assert (tab["q"][tab["q"] > 0] == 1).sum() == (tab["q"] > 0).sum() - 1


def test_sanitizer_program_runs_the_host_functions_on_degenerate_maps(tmp_path):
    """tests/sanitize/env_table_main.cpp, a program of its own built with ASan, UBSan and the float-cast-overflow check:
    bdpt_host_env_table, _sample and _eval on NaN / inf / negative / subnormal maps, an all-zero map, 1 x 1 and chunk-crossing
    sizes, with NaN, zero and infinite directions.  No conversion may be undefined and no access out of bounds."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    csrc = os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "csrc")
    exe = str(tmp_path / "env_table_main")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined,float-cast-overflow",
                        "-I", csrc, "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "sanitize", "env_table_main.cpp"),
                        os.path.join(csrc, "env_host.cpp")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "env table run finished failures=0" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


# ---- the host pass ---------------------------------------------------------------------------------------------------
def test_sky_pass_compiles_under_its_reference_style_name():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    host = os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "host")
    src = os.path.join(ROOT, "tests", "host_compile", "sky_pass_main.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + host, src],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "using namespace" not in open(src).read().split("int main")[1]


def test_bdpt_render_refuses_bad_sky_options(tmp_path):
    """--sky without --env FILE, N outside 1 .. 64, a clamp that is not > 0, --sky-clamp without --sky, and the switches only
    the replaced passes read exit non-zero with a message, before any GPU is touched"""
    render = os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "host", "bdpt_render")
    if not os.path.exists(render):
        pytest.skip("host/bdpt_render not built")
    env = ["--env", str(tmp_path / "probe.hdr")]
    for args, text in ((["--sky", "4"], "needs --env FILE"), (["--sky", "4", "--env", "Black"], "needs --env FILE"),
                       (env + ["--sky", "0"], "--sky N needs"), (env + ["--sky", "65"], "--sky N needs"), (env + ["--sky", "-2"], "--sky N needs"),
                       (env + ["--sky", "4", "--sky-clamp", "0"], "C > 0"), (env + ["--sky", "4", "--sky-clamp", "nan"], "C > 0"),
                       (env + ["--sky", "4", "--gpus", "1"], "one GPU"), (["--sky-clamp", "2"], "goes with --sky"),
                       (env + ["--sky", "4", "--denoise"], "not with --ao N"), (env + ["--sky", "4", "--ao", "2"], "not with --ao N"),
                       (env + ["--sky", "4", "--gi"], "not with --ao N")):
        r = subprocess.run([render] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and text in r.stderr, (args, r.stderr)
    u = subprocess.run([render, "--help"], capture_output=True, text=True, timeout=60)
    assert "--sky N [--sky-clamp C]" in u.stderr
