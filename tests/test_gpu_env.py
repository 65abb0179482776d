"""GPU tests of the environment map's sampling table and bdpt_env_query (csrc/env_light.hip): the device table against the
host table word for word, BDPT_ENV_SAMPLE against bdpt_host_env_sample plus the fp32 value arithmetic of tests/env_numpy.py,
BDPT_ENV_EVAL against the G-buffer miss shader's lookup and the host twin, compaction, capture, the error cases and the
table's lifetime.  Every comparison is on the words (floats viewed as integers; a NaN equals a NaN)."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library is loaded, as tests/test_gpu_gi.py: run alone, this module would otherwise load the library
#                first, and with it the system's copy of the HIP runtime beside the one torch ships, in which a graph captured on
#                a torch stream cannot be read back)

import edge_records as er
import env_numpy as en
from walk_loop import gpu, host

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
W, H = 64, 48
MISSES = 64
MIN_T = 1e-4
_state = {}


def words(a):
    """the words of a float array with every NaN made the same one"""
    a = np.ascontiguousarray(a, F)
    return np.where(np.isnan(a), U(0x7FC00000), a.view(U))


def bind(ctx, env):
    """upload `env` ((H, W, 4) float32), bind it and prepare its table; -> the device tensor (the map stays caller memory)"""
    t = gpu(np.ascontiguousarray(env, F))
    ctx.set_environment(t.data_ptr(), env.shape[1], env.shape[0])
    ctx.env_prepare()
    return t


def setup(pkg):
    """one Cornell pipeline at 64 x 48, its primary hits with miss records appended, seeds, and the maps with their host tables"""
    if "s" not in _state:
        from test_gpu_ao import _primary_items
        scene = pkg.Scene.cornell()
        pipe = pkg.FramePipeline(scene, W, H, max_depth=3, min_t=MIN_T)
        surf, seeds = _primary_items(pipe)
        lib = pkg.load_library()
        a = pkg.abi
        maps = {k: (env, en.host_table(lib, env)) for k, env in en.maps(a.ENV_ROW_SCAN_CHUNK, a.ENV_MARGINAL_CHUNK).items()}
        _state["s"] = dict(scene=scene, pipe=pipe, ctx=pipe.ctx, surf=surf, seeds=seeds, lib=lib, maps=maps)
    return _state["s"]


def test_device_table_equals_the_host_table(pkg):
    """every map of the CPU list, the two chunk-crossing sizes among them: cdf and rowCdf word for word, total, m and the
    chunk sizes through bdpt_get_env_info; a changed map of the same size is prepared again in place (same bytes, same
    addresses)"""
    s = setup(pkg)
    ctx, a = s["ctx"], pkg.abi
    for name, (env, tab) in s["maps"].items():
        t = bind(ctx, env)
        cdf, row = ctx.env_table()
        assert np.array_equal(cdf, tab["cdf"]) and np.array_equal(row, tab["row_cdf"]), name
        info = ctx.env_info()
        assert (info.width, info.height, info.total) == (env.shape[1], env.shape[0], tab["total"]), name
        assert F(info.max).view(U) == tab["m"].view(U), name
        assert (info.rowScanChunk, info.marginalChunk) == (a.ENV_ROW_SCAN_CHUNK, a.ENV_MARGINAL_CHUNK)
        assert info.tableBytes >= cdf.nbytes + row.nbytes
        if name in ("7x5", "sun", "wide2"):
            other = en.random_map(env.shape[1], env.shape[0], 99)
            other[0, 0, :3] = 0
            t.copy_(gpu(other))
            ctx.env_prepare()  # no set_environment: the same map memory, new contents
            cdf, row = ctx.env_table()
            want = en.host_table(s["lib"], other)
            assert np.array_equal(cdf, want["cdf"]) and np.array_equal(row, want["row_cdf"]), name
            again = ctx.env_info()
            assert (again.tableBytes, again.cdf, again.rowCdf) == (info.tableBytes, info.cdf, info.rowCdf), name
            assert again.total == want["total"] != info.total
    ctx.set_environment()


def _sample(ctx, surf, seeds, mat, compact=None, count=None, fill=-7):
    import torch
    n = len(surf)
    out = torch.full((n, 20), float(fill), dtype=torch.float32, device="cuda")
    sout = torch.full((n,), int(fill), dtype=torch.int32, device="cuda")
    ctx.env_sample(gpu(surf), gpu(np.ascontiguousarray(seeds, U).view(np.int32)), mat_index=mat, min_t=MIN_T, out=out, seeds_out=sout,
                   compact=compact, count=count)
    torch.cuda.synchronize()
    return host(out), host(sout).view(U)


def _expected_sample(lib, env, tab, surf, seeds, mat):
    """bdpt_host_env_sample plus the numpy value arithmetic -> the (n, 20) words and the states after four draws"""
    got, after = en.host_sample(lib, env, tab, seeds)
    n = len(surf)
    N, V, dif, spec = surf[:, 4:7], surf[:, 8:11], surf[:, 12:15], surf[:, 16:19]
    if mat == 1:
        value = en.lambert_value(N, got["dir"], got["radiance"], dif, got["pdf"])
    else:
        value = en.ggx_value(N, V, got["dir"], got["radiance"], dif, spec, surf[:, 7], got["pdf"])
    want = np.zeros((n, 20), F)
    want[:, 0:3], want[:, 3], want[:, 4:7], want[:, 7] = surf[:, 0:3], F(MIN_T), got["dir"], F(1e38)
    want[:, 8:11], want[:, 11], want[:, 12:15] = got["radiance"], got["pdf"], value
    want.view(U)[:, 15] = got["texel"]
    with np.errstate(invalid="ignore"):
        want.view(U)[:, 16] = (~(value == 0).all(axis=1)).astype(U)
    want[surf.view(np.int32)[:, 23] < 0] = 0
    return want, after


def _records(s):
    """the Cornell items, then records of tests/edge_records.py (degenerate N, colours and roughness, prim < 0), then a few
    with a NaN or infinite posW"""
    mixed = er.bsdf_mixed()
    edge = mixed.surf[:512].copy()
    extra = s["surf"][:8].copy()
    extra[0:3, 0] = F("nan")
    extra[3:5, 0:3] = F("inf")
    extra[5, 4:7] = 0
    extra[6, 4:7] = F("nan")
    extra.view(np.int32)[7, 23] = -1
    surf = np.concatenate([s["surf"], edge, extra])
    rng = np.random.default_rng(4)
    return surf, rng.integers(0, 2**32, len(surf), dtype=np.uint64).astype(U)


@pytest.mark.parametrize("name", ["sun", "7x5", "edge", "zero"])
def test_sample_equals_the_host_sampler_and_the_numpy_value(pkg, name):
    """every item, matIndex 0 and 1: the five float4 of bdpt_env_sample and seedsOut (four LCG steps)"""
    s = setup(pkg)
    ctx = s["ctx"]
    env, tab = s["maps"][name]
    keep = bind(ctx, env)
    surf, seeds = _records(s)
    assert (surf.view(np.int32)[:, 23] < 0).sum() >= MISSES
    for mat in (1, 0):
        got, sout = _sample(ctx, surf, seeds, mat)
        want, after = _expected_sample(s["lib"], env, tab, surf, seeds, mat)
        assert np.array_equal(sout, after) and np.array_equal(after, en.draws(seeds)[1])
        for lo, hi, what in ((0, 8, "ray"), (8, 12, "radiance / pdf"), (12, 15, "value"), (15, 20, "texel / status")):
            bad = (words(got[:, lo:hi]) != words(want[:, lo:hi])).any(axis=1)
            assert not bad.any(), f"{name} matIndex {mat}: {what} differ in {int(bad.sum())} of {len(bad)} items, first {int(np.argmax(bad))}"
        if name == "zero":
            assert not got[:, 4:7].view(U).any() and not got[:, 8:17].view(U).any()  # no direction, radiance, pdf, value or status
        else:
            assert (got.view(U)[:, 16] == 1).any() and (got.view(U)[:, 16] == 0).any()
    del keep
    ctx.set_environment()


def test_compaction_and_device_counts(pkg):
    """the compacted list holds exactly the NONZERO items with their rays; items at or beyond the device count are untouched"""
    import torch
    s = setup(pkg)
    ctx = s["ctx"]
    env, tab = s["maps"]["7x5"]
    keep = bind(ctx, env)
    surf, seeds = s["surf"], s["seeds"]
    n = len(surf)
    plain, _ = _sample(ctx, surf, seeds, 1)
    rays = torch.full((n, 8), -7.0, dtype=torch.float32, device="cuda")
    items = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    cc = torch.zeros(1, dtype=torch.int32, device="cuda")
    got, _ = _sample(ctx, surf, seeds, 1, compact=(rays, items, cc))
    assert np.array_equal(words(got), words(plain))
    k = int(host(cc)[0])
    nz = np.nonzero(plain.view(U)[:, 16] == 1)[0]
    it = host(items)[:k]
    assert k == len(nz) and 0 < k < n and np.array_equal(np.sort(it), nz)
    assert np.array_equal(words(host(rays)[:k]), words(plain[it, 0:8]))
    assert (host(items)[k:] == -7).all() and (host(rays)[k:] == -7).all()
    for m in (0, 1, 63, 64, 65, n + 5):
        cnt = torch.tensor([m], dtype=torch.int32, device="cuda")
        got, sout = _sample(ctx, surf, seeds, 0, count=cnt)
        kk = min(m, n)
        assert (got[kk:] == -7).all() and (sout.view(np.int32)[kk:] == -7).all(), m
        assert np.array_equal(sout[:kk], en.draws(seeds[:kk])[1])
    # in place: seeds_out may be seeds
    st = gpu(seeds.view(np.int32))
    ctx.env_sample(gpu(surf), st, seeds_out=st)
    torch.cuda.synchronize()
    assert np.array_equal(host(st).view(U), en.draws(seeds)[1])
    del keep
    ctx.set_environment()


def _index_map(w, h):
    """radiance = (texel index + 1, x, y): whole numbers up to 2048, which the G-buffer's half channel holds exactly; no texel
    is black, so a lookup outside the map (0) is told from every texel"""
    env = np.ones((h, w, 4), F)
    yy, xx = np.mgrid[0:h, 0:w]
    env[..., 0], env[..., 1], env[..., 2] = yy * w + xx + 1, xx, yy
    return env


def test_eval_equals_the_gbuffer_miss_shader_and_the_host_twin(pkg):
    """(a) cameras outside the box looking away from it: the G-buffer pass's miss pixels hold envLookup of their primary ray;
    bdpt_env_query(EVAL) of those rays' directions returns that texel and radiance exactly; cameras with a NaN and with an
    all-zero basis give every pixel a NaN primary direction, which the miss shader and EVAL both look up as texel (W / 2, 0) with pdf 0 (atan2_WAR of NaNs is 0, so u = 0.5; the
    device's float to integer conversion; include/bdpt.h says so).  (b) sampled, random, zero, NaN
    and infinite directions: radiance, pdf and texel equal bdpt_host_env_eval's, word for word"""
    import torch
    s = setup(pkg)
    pipe, ctx, lib, a = s["pipe"], s["ctx"], s["lib"], pkg.abi
    env = _index_map(64, 32)
    tab = en.host_table(lib, env)
    t = bind(ctx, env)
    v3 = lambda x: (C.c_float * 3)(*x)
    seen = set()
    for look in ((1, 0, 0), (-1, 0, 0), (0, 1, 0.01), (0, -1, 0.01), (0, 0, 1), (0, 0, -1), (1, 1, 1), (-1, -0.5, 0.25), "nan", "zero"):
        cam = a.Camera()
        if isinstance(look, str):  # every primary direction is NaN (normalize of a NaN or of a zero vector)
            for k in range(3):
                cam.posW[k] = 5000.0
                cam.cameraU[k] = cam.cameraV[k] = 0.0
                cam.cameraW[k] = float("nan") if look == "nan" else 0.0
        else:
            pos = np.array([278.0, 273.0, -800.0]) + 5000.0 * np.array(look)
            assert lib.bdpt_camera_look_at(v3(pos), v3(pos + np.array(look)), v3((0.0, 1.0, 0.0)), 10.0, 24.0, W / H, 1.0, C.byref(cam)) == 0
        ctx.set_camera(cam)
        gp = pipe.gbuffer_params()
        gp.envMap, gp.envWidth, gp.envHeight = t.data_ptr(), 64, 32
        rays = ctx.camera_rays(gp, W, H)
        ctx.gbuffer_execute(gp, pipe.gb)
        dirs = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
        dirs[:, 0:3] = rays[:, 4:7]
        ev = ctx.env_eval(dirs)
        torch.cuda.synchronize()
        miss = host(pipe.channels["WorldPosition"]).reshape(-1, 4)[:, 3] == 0
        dif = host(pipe.channels["MaterialDiffuse"].float()).reshape(-1, 4)
        ev = host(ev)
        inside = ev.view(U)[:, 4] != a.ENV_NO_TEXEL
        assert miss.mean() > 0.9
        assert np.array_equal(ev[miss, 0:3], dif[miss, 0:3])
        assert np.array_equal(ev.view(U)[miss & inside, 4], dif[miss & inside, 0].astype(U) - 1) and (dif[miss & inside, 0] >= 1).all()
        assert (dif[miss & ~inside, 0:3] == 0).all()
        if isinstance(look, str):
            assert np.isnan(host(rays)[:, 4:7]).all() and miss.all(), look
            assert (ev.view(U)[:, 4] == 32).all() and (dif[:, 0:3] == np.array([33, 32, 0], F)).all() and (ev[:, 3] == 0).all(), look
            continue
        seen |= set(ev.view(U)[miss & inside, 4].tolist())
    assert len(seen) > 1000  # most of the map's 2048 texels were looked up
    ctx.set_camera(pipe.cam)
    # (b)
    rng = np.random.default_rng(8)
    nan, inf = F("nan"), F("inf")
    for name in ("sun", "7x5", "edge"):
        env, tab = s["maps"][name]
        keep = bind(ctx, env)
        sampled, _ = en.host_sample(lib, env, tab, rng.integers(0, 2**32, 2048, dtype=np.uint64).astype(U))
        odd = np.array([(0, 0, 0), (-0.0, 0, -0.0), (nan, 0, 1), (0, nan, 0), (1, 0, nan), (nan, nan, nan), (inf, 0, 0), (0, -inf, 0), (0, 1, 0),
                        (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 0, 0), (-1, 0, 0), (0.0, 0.5, 1.0), (-0.0, 0.5, 1.0), (1e-30, 0, 1e-30), (1e20, 1e20, 1e20)], F)
        d = np.concatenate([sampled["dir"], rng.normal(size=(2048, 3)).astype(F), odd])
        d4 = np.concatenate([d, rng.normal(size=(len(d), 1)).astype(F)], axis=1)  # (w is not read)
        got = host(ctx.env_eval(gpu(d4)))
        torch.cuda.synchronize()
        want = en.host_eval(lib, env, tab, d)
        assert np.array_equal(words(got[:, 0:3]), words(want["radiance"])), name
        assert np.array_equal(got[:, 3].view(U), want["pdf"].view(U)), name
        assert np.array_equal(got.view(U)[:, 4], want["texel"]) and not got.view(U)[:, 5:8].any(), name
        outside = want["texel"] == a.ENV_NO_TEXEL
        assert outside.any() and not got[outside, 0:4].view(U).any()
        assert (got.view(U)[:len(sampled), 4] == sampled["texel"]).mean() > 0.99  # a sampled direction looks up its own texel
        del keep
    ctx.set_environment()


def test_captured_prepare_and_query(pkg):
    """a repeat bdpt_env_prepare of the same size is captured with a sample query behind it, without an allocation; replayed
    after the map changed, the table is the new map's and the samples are the host's.  The graph holds four kernel nodes."""
    from test_gpu_walk_query import _graph_node_types
    s = setup(pkg)
    ctx, lib = s["ctx"], s["lib"]
    env = s["maps"]["7x5"][0]
    t = bind(ctx, env)
    surf, seeds = gpu(s["surf"]), gpu(s["seeds"].view(np.int32))
    out = torch.zeros((len(s["surf"]), 20), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        st = C.c_void_p(side.cuda_stream)
        ctx.env_prepare(st)  # eagerly first: the context's last stream is then the capturing one
        side.synchronize()
        pad = torch.zeros(1, device="cuda")
        trivial = torch.cuda.CUDAGraph()  # (what torch itself allocates for a first capture is behind us after this one)
        trivial.capture_begin()
        pad.add_(1)
        trivial.capture_end()
        alloc = torch.cuda.memory_allocated()
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        graph.capture_begin()
        ctx.env_prepare(st)
        ctx.env_sample(surf, seeds, mat_index=1, min_t=MIN_T, out=out, stream=st)
        graph.capture_end()
        assert torch.cuda.memory_allocated() == alloc
    torch.cuda.synchronize()
    assert (host(out) == 0).all()  # captured, not run
    assert _graph_node_types(graph) == [0, 0, 0, 0]  # the table's three kernels and the query's: no memset, no copy, no host node
    for seed in (50, 51):
        other = en.random_map(7, 5, seed)
        t.copy_(gpu(other))
        graph.replay()
        torch.cuda.synchronize()
        tab = en.host_table(lib, other)
        cdf, row = ctx.env_table()
        assert np.array_equal(cdf, tab["cdf"]) and np.array_equal(row, tab["row_cdf"])
        want, _ = _expected_sample(lib, other, tab, s["surf"], s["seeds"], 1)
        assert np.array_equal(words(host(out)), words(want))
    del graph, trivial
    ctx.set_environment()


def test_error_cases_and_the_tables_lifetime(pkg):
    """every error case returns its code in the documented order, nothing is enqueued (the outputs keep their sentinel), and
    bdpt_set_environment drops the table"""
    import torch
    a = pkg.abi
    lib = pkg.load_library()
    ctx = pkg.Context(0)
    n = 256
    surf = torch.zeros((n, 24), dtype=torch.float32, device="cuda")
    seeds = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = torch.full((n, 20), -7.0, dtype=torch.float32, device="cuda")
    ev = torch.full((n, 8), -7.0, dtype=torch.float32, device="cuda")
    dirs = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    cr, ci, cc = (torch.full((n, 8), -7.0, device="cuda"), torch.full((n,), -7, dtype=torch.int32, device="cuda"),
                  torch.zeros(1, dtype=torch.int32, device="cuda"))
    env = gpu(en.random_map(7, 5, 4))
    P = dict(sf=surf.data_ptr(), sd=seeds.data_ptr(), out=out.data_ptr(), ev=ev.data_ptr(), d=dirs.data_ptr(), cr=cr.data_ptr(), ci=ci.data_ptr(),
             cc=cc.data_ptr())

    def q(h=ctx._h, mode=0, num=n, mat=1, flags=0, reserved=0, cnt=None, sf=P["sf"], sd=P["sd"], so=None, smp=P["out"], d=None, evals=None,
          comp=(None, None, None), desc=True):
        e = a.EnvDesc()
        e.mode, e.num, e.numDevice, e.matIndex, e.flags, e.minT, e.reserved = mode, num, cnt, mat, flags, 1e-4, reserved
        e.surfaces, e.seeds, e.seedsOut, e.samples, e.dirs, e.evals = sf, sd, so, smp, d, evals
        e.compactRays, e.compactItems, e.compactCount = comp
        return lib.bdpt_env_query(h, C.byref(e) if desc else None, None)

    assert lib.bdpt_env_prepare(ctx._h, None) == -2 and b"env_prepare" in lib.bdpt_last_error(ctx._h)  # no environment at all
    ctx.set_environment(color=(0.5, 0.5, 0.8, 1.0))
    assert lib.bdpt_env_prepare(ctx._h, None) == -2  # a constant colour is no map
    assert q() == -2 and b"env_query" in lib.bdpt_last_error(ctx._h) and b"no environment map" in lib.bdpt_last_error(ctx._h)
    assert q(mode=7) == -2  # the state comes first
    info = a.EnvInfo()
    assert lib.bdpt_get_env_info(ctx._h, C.byref(info)) == -2
    ctx.set_environment(env.data_ptr(), 7, 5)
    assert q() == -2 and b"bdpt_env_prepare first" in lib.bdpt_last_error(ctx._h)  # a map, but no table yet
    big = a.Environment()
    big.envMap, big.width, big.height = env.data_ptr(), 16385, 1
    assert lib.bdpt_set_environment(ctx._h, C.byref(big)) == 0 and lib.bdpt_env_prepare(ctx._h, None) == -5  # BDPT_E_LIMIT
    big.width, big.height = 1, 16385
    assert lib.bdpt_set_environment(ctx._h, C.byref(big)) == 0 and lib.bdpt_env_prepare(ctx._h, None) == -5
    ctx.set_environment(env.data_ptr() + 4, 7, 4)
    assert lib.bdpt_env_prepare(ctx._h, None) == -1  # a map that is not 16-byte aligned
    ctx.set_environment(env.data_ptr(), 7, 5)
    ctx.env_prepare()
    full = (P["cr"], P["ci"], P["cc"])
    bad = [
        q(h=None), q(desc=False), q(mode=2), q(mat=2), q(flags=1), q(reserved=1), q(num=0, mode=9), q(comp=(P["cr"], None, None)),
        q(comp=(P["cr"], P["ci"], None)), q(num=0, comp=(None, P["ci"], P["cc"])), q(mode=1, d=P["d"], evals=P["ev"], comp=full),
        q(sf=None), q(sf=P["sf"] + 4), q(sd=None), q(sd=P["sd"] + 2), q(smp=None), q(smp=P["out"] + 8), q(so=P["sd"] + 1), q(cnt=P["cc"] + 2),
        q(comp=(P["cr"] + 8, P["ci"], P["cc"])), q(comp=(P["cr"], P["ci"] + 2, P["cc"])), q(mode=1, d=None, evals=P["ev"]),
        q(mode=1, d=P["d"] + 4, evals=P["ev"]), q(mode=1, d=P["d"], evals=None), q(mode=1, d=P["d"], evals=P["ev"] + 8),
    ]
    assert all(rc == -1 for rc in bad), bad
    assert b"env_query" in lib.bdpt_last_error(ctx._h)
    assert q(num=0, sf=None, sd=None, smp=None) == 0
    torch.cuda.synchronize()
    for t in (out, ev, cr, ci):
        assert (host(t) == -7).all()
    # the good calls, then the lifetime: set_environment drops the table (with the same map, a cleared one, a colour)
    assert q(so=P["sd"], comp=full) == 0 and q(mode=1, d=P["d"], evals=P["ev"]) == 0
    torch.cuda.synchronize()
    assert (host(out) != -7).all() and (host(ev) != -7).all()
    for again in (lambda: ctx.set_environment(env.data_ptr(), 7, 5), lambda: ctx.set_environment(), lambda: ctx.set_environment(color=(1, 1, 1, 1))):
        ctx.set_environment(env.data_ptr(), 7, 5)
        ctx.env_prepare()
        assert q() == 0 and lib.bdpt_get_env_info(ctx._h, C.byref(info)) == 0 and info.width == 7
        again()
        assert q() == -2 and lib.bdpt_get_env_info(ctx._h, C.byref(info)) == -2
        assert lib.bdpt_test_env_table(ctx._h, P["cr"], P["ci"]) == -2
    # the first prepare for a size allocates: refused inside a capture, and the capture stays usable
    ctx.set_environment(env.data_ptr(), 7, 5)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        pad = torch.zeros(1, device="cuda")
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        g.capture_begin()
        pad.add_(1)
        rc = lib.bdpt_env_prepare(ctx._h, C.c_void_p(side.cuda_stream))
        g.capture_end()
    assert rc == -2 and b"capture" in lib.bdpt_last_error(ctx._h)
    torch.cuda.synchronize()
    ctx.close()
