"""GPU tests of sky lighting (csrc/sky.hip): bdpt_sky_query and bdpt_sky_execute against the composed device loop they replace
(per sample env_sample(mat_index=1) -> clamp -> trace_rays("any") -> an ordered add of the visible non-zero terms), bit for
bit — colour words, counts and states over every item — plus tiles, capture, convergence to a float64 quadrature, the error
cases and the host pass."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch  # (before the library is loaded: see tests/test_gpu_env.py)

import ao_reference as ar
import env_numpy as en
from area_scenes import bits
from test_gpu_env import H, MIN_T, W, bind, setup
from walk_loop import gpu, host

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
FLT_MAX = float(en.FLT_MAX)
SNAPSHOTS = (1, 2, 64)


def sky_loop(ctx, surf, seeds, clamp, alive=None, snapshots=SNAPSHOTS):
    """The composed loop on the device, one stream: numpy in, {samples: (color (n, 4), counts, seeds_out)} out for every sample
    count of `snapshots` (the state after k samples is the k-sample answer but for the final division)."""
    import torch
    surf_t, s = gpu(surf), gpu(np.ascontiguousarray(seeds, U).view(np.int32))
    n = surf_t.shape[0]
    live = surf_t.view(torch.int32)[:, 23] >= 0
    if alive is not None:
        live = live & (gpu(alive) != 0)
    hi = torch.tensor(clamp, dtype=torch.float32, device="cuda")
    zero = torch.zeros((), dtype=torch.float32, device="cuda")
    total = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    smp = torch.empty((n, 20), dtype=torch.float32, device="cuda")
    nxt = torch.empty(n, dtype=torch.int32, device="cuda")
    vis = torch.empty(n, dtype=torch.uint8, device="cuda")
    out = {}
    for k in range(1, max(snapshots) + 1):
        ctx.env_sample(surf_t, s, mat_index=1, min_t=MIN_T, out=smp, seeds_out=nxt)
        v = smp[:, 12:15]
        y = torch.where(v > 0, v, zero)
        value = torch.where(y < hi, y, hi)  # clampVec
        ctx.trace_rays(smp[:, 0:8].contiguous(), "any", out=vis)
        add = live & (value != 0).any(dim=1) & (vis != 0)  # a non-zero term whose ray is unoccluded
        total = total + torch.where(add[:, None], value, zero)
        cnt = cnt + add.to(torch.int32)
        s = torch.where(live, nxt, s)
        if k in snapshots:
            color = torch.ones((n, 4), dtype=torch.float32, device="cuda")
            color[:, 0:3] = torch.where(live[:, None], total / float(k), surf_t[:, 12:15])
            torch.cuda.synchronize()
            out[k] = (host(color), host(cnt).view(U).copy(), host(s).view(U).copy())
    return out


def sky_query(ctx, surf, seeds, samples, clamp, alive=None, count=None, fill=-7):
    import torch
    n = len(surf)
    col = torch.full((n, 4), float(fill), dtype=torch.float32, device="cuda")
    counts = torch.full((n,), int(fill), dtype=torch.int32, device="cuda")
    sout = torch.full((n,), int(fill), dtype=torch.int32, device="cuda")
    res = ctx.sky_lighting(gpu(surf), gpu(np.ascontiguousarray(seeds, U).view(np.int32)), samples, clamp=clamp, min_t=MIN_T,
                           alive=None if alive is None else gpu(alive), out=col, counts=counts, seeds_out=sout, count=count)
    assert res is col
    torch.cuda.synchronize()
    return host(col), host(counts).view(U), host(sout).view(U)


def _assert_same(got, want, what):
    for name, g, w in zip(("color", "counts", "seeds_out"), got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        diff = g.view(U) != w.view(U)
        assert not diff.any(), f"{what}: {name} differ in {int(diff.sum())} of {diff.size} words, first item {int(np.argmax(diff.reshape(len(g), -1).any(axis=1)))}"


_loops = {}


def _loop_of(s, name, clamp):
    """the composed loop's answers for map `name` (bound by the caller), computed once per (map, clamp) and shared"""
    key = (name, repr(clamp))
    if key not in _loops:
        _loops[key] = sky_loop(s["ctx"], s["surf"], s["seeds"], clamp)
    return _loops[key]


@pytest.mark.parametrize("name", ["sun", "7x5"])
def test_equals_the_composed_loop(pkg, name):
    """samples 1, 2 and 64, clampUpper 1 and FLT_MAX: colour words, counts and states of every item equal the loop's"""
    s = setup(pkg)
    ctx, surf, seeds = s["ctx"], s["surf"], s["seeds"]
    keep = bind(ctx, s["maps"][name][0])
    lv = surf.view(np.int32)[:, 23] >= 0
    for clamp in (1.0, FLT_MAX):
        want = _loop_of(s, name, clamp)
        for samples in SNAPSHOTS:
            got = sky_query(ctx, surf, seeds, samples, clamp)
            _assert_same(got, want[samples], f"{name} S {samples} clamp {clamp}")
            color, counts, sout = got
            assert np.array_equal(color[~lv, 0:3].view(U), surf[~lv, 12:15].view(U)) and (counts[~lv] == 0).all()
            assert np.array_equal(sout[~lv], seeds[~lv]) and np.array_equal(sout[lv], en.draws(seeds[lv], 4 * samples)[1])
            assert (color[:, 3] == 1.0).all() and (counts <= samples).all()
            if clamp == 1.0:
                assert (color[lv, 0:3] <= 1.0).all()
        assert (want[64][1][lv] > 0).any() and (want[64][1][lv] < 64).any()  # lit and shadowed samples both occur
    if name == "sun":
        assert not np.array_equal(_loop_of(s, name, 1.0)[64][0], _loop_of(s, name, FLT_MAX)[64][0])  # the clamp bites
    del keep
    ctx.set_environment()


def test_alive_masks_device_counts_and_item_counts(pkg):
    """alive bytes that drop every third item; device counts below, at and above num with the words beyond untouched; 1, 63,
    64, 65 items"""
    import torch
    s = setup(pkg)
    ctx, surf, seeds = s["ctx"], s["surf"], s["seeds"]
    keep = bind(ctx, s["maps"]["7x5"][0])
    n, S = len(surf), 2
    want = _loop_of(s, "7x5", FLT_MAX)[S]
    for m in (1, 63, 64, 65):
        _assert_same(sky_query(ctx, surf[:m], seeds[:m], S, FLT_MAX), [w[:m] for w in want], f"{m} items")
    for m in (0, 1, 63, 64, 65, n, n + 9):
        cnt = torch.tensor([m], dtype=torch.int32, device="cuda")
        got = sky_query(ctx, surf, seeds, S, FLT_MAX, count=cnt)
        k = min(m, n)
        _assert_same([g[:k] for g in got], [w[:k] for w in want], f"device count {m}")
        assert (got[0][k:] == -7.0).all() and (got[1].view(np.int32)[k:] == -7).all() and (got[2].view(np.int32)[k:] == -7).all(), m
    alive = (np.arange(n) % 3 != 1).astype(np.uint8)
    got = sky_query(ctx, surf, seeds, S, FLT_MAX, alive=alive)
    _assert_same(got, sky_loop(ctx, surf, seeds, FLT_MAX, alive=alive, snapshots=(S,))[S], "alive")
    dead = alive == 0
    assert np.array_equal(got[0][dead, 0:3].view(U), surf[dead, 12:15].view(U)) and (got[1][dead] == 0).all()
    assert np.array_equal(got[2][dead], seeds[dead])
    # in place: seeds_out may be seeds; host arrays go to the device and back
    st = gpu(seeds.view(np.int32))
    ctx.sky_lighting(gpu(surf), st, S, min_t=MIN_T, seeds_out=st)
    torch.cuda.synchronize()
    assert np.array_equal(host(st).view(U), want[2])
    h = ctx.sky_lighting(surf[:65], seeds[:65], S, min_t=MIN_T)
    assert isinstance(h, np.ndarray) and np.array_equal(h.view(U), want[0][:65].view(U))
    del keep
    ctx.set_environment()


def test_all_zero_map(pkg):
    """total == 0: colour 0, every draw taken, no sample counted"""
    s = setup(pkg)
    ctx, surf, seeds = s["ctx"], s["surf"], s["seeds"]
    keep = bind(ctx, s["maps"]["zero"][0])
    lv = surf.view(np.int32)[:, 23] >= 0
    for samples in (1, 64):
        color, counts, sout = sky_query(ctx, surf, seeds, samples, FLT_MAX)
        assert not color[lv, 0:3].view(U).any() and (color[:, 3] == 1.0).all() and not counts.any()
        assert np.array_equal(sout[lv], en.draws(seeds[lv], 4 * samples)[1]) and np.array_equal(sout[~lv], seeds[~lv])
    del keep
    ctx.set_environment()


def _gbuffer_records(pipe, frame):
    """the query's inputs for the pass: positions, half-decoded normals and diffuse, prim from worldPosition.w, the pass's seeds"""
    from test_gpu_ao import _gbuffer_items
    rec, seeds = _gbuffer_items(pipe, frame)
    rec[:, 12:15] = host(pipe.channels["MaterialDiffuse"].float()).reshape(-1, 4)[:, 0:3]
    return rec, seeds


def test_execute_equals_the_query_and_tiles_reproduce_the_frame(pkg):
    """bdpt_sky_execute equals the query fed the G-buffer; two row tiles and a stripes context write only their pixels, with
    the whole frame's values; the frame counter advances by one per call"""
    import torch
    s = setup(pkg)
    pipe, ctx, a = s["pipe"], s["ctx"], pkg.abi
    env_t = bind(ctx, s["maps"]["7x5"][0])
    st = pipe._stream_ptr()
    ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, st)
    torch.cuda.synchronize()
    S, clamp = 4, 2.0
    images = {}
    for frame in (0, 0, 5):
        pipe.sky_frame = frame
        img = host(pipe.sky_lighting(S, clamp)).copy()
        assert pipe.sky_frame == frame + 1 and pipe.last_sky_params.frameCount == frame
        if frame in images:
            assert np.array_equal(bits(img), bits(images[frame]))
        images[frame] = img
    assert not np.array_equal(bits(images[0]), bits(images[5]))
    for frame, img in images.items():
        rec, seeds = _gbuffer_records(pipe, frame)
        color, _, _ = sky_query(ctx, rec, seeds, S, clamp)
        assert np.array_equal(bits(img), bits(color.reshape(H, W, 4))), frame
        background = rec.view(np.int32)[:, 23] < 0
        assert background.any() and (color[~background, 0:3] > 0).any()
    p = a.SkyParams(0, clamp, MIN_T, S, 0)
    for kind, args in (("rows", (0, 16)), ("rows", (16, H)), ("stripes", None)):
        tile = pkg.Context(0)
        tile.set_scene(s["scene"].desc)
        if kind == "rows":
            tile.resize(W, H, args[0], args[1], 3)
        else:
            tile.resize_stripes(W, H, 4, 3, 1, 3)
        tile.set_environment(env_t.data_ptr(), 7, 5)
        tile.env_prepare()
        rows = np.zeros(H, bool)
        for y0, y1 in tile.row_ranges():
            rows[y0:y1] = True
        assert 0 < rows.sum() < H
        out = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
        tile.sky_execute(p, pipe.gb, C.c_void_p(out.data_ptr()), st)  # (no camera set: the pass needs none)
        torch.cuda.synchronize()
        got = host(out)
        assert np.array_equal(bits(got[rows]), bits(images[0][rows])), kind
        assert (got[~rows] == -7.0).all(), kind
        tile.close()
    ctx.set_environment()


def test_captured_sky_execute(pkg):
    """bdpt_sky_execute captured for two consecutive frame counters: each graph holds exactly one kernel node, capturing
    allocates nothing, and two replays of each equal the eager call"""
    import torch
    from test_gpu_ao import _captured_once
    s = setup(pkg)
    pipe, ctx = s["pipe"], s["ctx"]
    keep = bind(ctx, s["maps"]["7x5"][0])
    ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, pipe._stream_ptr())
    torch.cuda.synchronize()
    img = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    frames = []
    for frame in (3, 4):
        p = pkg.abi.SkyParams(frame, FLT_MAX, MIN_T, 4, 0)
        eager = _captured_once(lambda st: ctx.sky_execute(p, pipe.gb, C.c_void_p(img.data_ptr()), st), dict(img=img), [0])
        rec, seeds = _gbuffer_records(pipe, frame)
        color, _, _ = sky_query(ctx, rec, seeds, 4, FLT_MAX)
        assert np.array_equal(bits(host(eager["img"])), bits(color.reshape(H, W, 4)))
        frames.append(host(eager["img"]).copy())
    assert not np.array_equal(bits(frames[0]), bits(frames[1]))
    del keep
    ctx.set_environment()


def test_converges_to_the_float64_quadrature(pkg):
    """an unoccluded upward-facing white item above the box under the 7 x 5 map, 64 samples x 256 seeds: the mean lies within 5
    standard errors (from the 256 estimates themselves) of sum over texels radiance * integral of cos / pi over the texel"""
    s = setup(pkg)
    ctx = s["ctx"]
    env = s["maps"]["7x5"][0]
    keep = bind(ctx, env)
    n = 256
    rec = ar.surface_records(np.tile(np.array([[278.0, 700.0, 280.0]], F), (n, 1)), np.tile(np.array([[0, 1, 0]], F), (n, 1)))
    rec[:, 12:15] = 1.0
    seeds = np.random.default_rng(77).integers(0, 2**32, n, dtype=np.uint64).astype(U)
    color, counts, _ = sky_query(ctx, rec, seeds, 64, FLT_MAX)
    hh, ww = env.shape[:2]
    th0, th1 = np.pi * np.arange(hh) / hh, np.pi * (np.arange(hh) + 1) / hh
    th0, th1 = np.minimum(th0, np.pi / 2), np.minimum(th1, np.pi / 2)  # N = +y: the upper hemisphere
    weight = (np.sin(th1) ** 2 - np.sin(th0) ** 2) / ww  # integral of cos(theta) / pi over a texel of row y
    want = (env[..., :3].astype(np.float64) * weight[:, None, None]).sum(axis=(0, 1))
    est = color[:, 0:3].astype(np.float64)
    mean, sem = est.mean(axis=0), est.std(axis=0, ddof=1) / math.sqrt(n)
    print(f"quadrature {want}, mean of {n} estimates {mean}, standard error {sem}, unoccluded {counts.mean():.1f} of 64")
    assert (sem > 0).all() and (np.abs(mean - want) <= 5 * sem).all(), (mean, want, sem)
    assert (counts > 0).all()
    del keep
    ctx.set_environment()


def test_error_cases_through_the_c_abi(pkg):
    """every error case in the documented order, nothing enqueued: no scene, no size, a stale table, no map, samples 0 and 65,
    flags, reserved, misaligned buffers"""
    import torch
    a = pkg.abi
    lib = pkg.load_library()
    s = setup(pkg)
    ctx = pkg.Context(0)
    n = 256
    surf = torch.zeros((n, 24), dtype=torch.float32, device="cuda")
    seeds = torch.zeros(n, dtype=torch.int32, device="cuda")
    alive = torch.ones(n, dtype=torch.uint8, device="cuda")
    cnt = torch.full((4,), n, dtype=torch.int32, device="cuda")
    col = torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda")
    outs = {k: torch.full((n,), -7, dtype=torch.int32, device="cuda") for k in ("c", "so")}
    img = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
    gpos = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    gh = torch.zeros((2, H, W, 4), dtype=torch.float16, device="cuda")
    env = gpu(en.random_map(7, 5, 4))
    P = dict(sf=surf.data_ptr(), sd=seeds.data_ptr(), b=alive.data_ptr(), n=cnt.data_ptr(), col=col.data_ptr(), img=img.data_ptr(),
             gp=gpos.data_ptr(), gn=gh[0].data_ptr(), gd=gh[1].data_ptr(), **{k: t.data_ptr() for k, t in outs.items()})

    def q(h=ctx._h, num=n, samples=4, cnt=None, flags=0, reserved=0, sf=P["sf"], sd=P["sd"], al=None, color=P["col"], c=None, so=None, desc=True):
        d = a.SkyDesc()
        d.num, d.samples, d.numDevice, d.clampUpper, d.minT, d.flags, d.reserved = num, samples, cnt, 10.0, 1e-4, flags, reserved
        d.surfaces, d.seeds, d.alive, d.color, d.counts, d.seedsOut = sf, sd, al, color, c, so
        return lib.bdpt_sky_query(h, C.byref(d) if desc else None, None)

    def x(h=ctx._h, samples=4, reserved=0, gp=P["gp"], gn=P["gn"], gd=P["gd"], out=P["img"], params=True, gbuffer=True):
        p = a.SkyParams(0, 10.0, 1e-4, samples, reserved)
        gb = a.GBuffer()
        gb.worldPosition, gb.worldNormal, gb.materialDiffuse = gp, gn, gd
        return lib.bdpt_sky_execute(h, C.byref(p) if params else None, C.byref(gb) if gbuffer else None, out, None)

    assert q() == -2 and b"sky_query" in lib.bdpt_last_error(ctx._h) and b"no scene" in lib.bdpt_last_error(ctx._h)
    assert x() == -2 and b"sky_execute" in lib.bdpt_last_error(ctx._h)
    ctx.set_scene(s["scene"].desc)
    assert q() == -2 and b"no environment map" in lib.bdpt_last_error(ctx._h)  # a scene, but no map
    assert q(samples=0) == -2  # the state comes first
    assert x() == -2 and b"no size" in lib.bdpt_last_error(ctx._h)
    ctx.resize(W, H, 0, H, 3)
    assert x() == -2 and b"no environment map" in lib.bdpt_last_error(ctx._h)
    ctx.set_environment(env.data_ptr(), 7, 5)
    assert q() == -2 and x() == -2 and b"bdpt_env_prepare first" in lib.bdpt_last_error(ctx._h)  # a map, but no table
    ctx.env_prepare()
    ctx.set_environment(env.data_ptr(), 7, 5)  # the table goes stale with a new environment, even the same one
    assert q() == -2 and x(samples=0) == -2
    ctx.env_prepare()
    bad = [
        q(h=None), q(desc=False), q(samples=0), q(samples=65), q(samples=2**31), q(flags=1), q(reserved=1), q(num=0, samples=0),
        q(num=0, flags=8), q(sf=None), q(sf=P["sf"] + 4), q(sd=None), q(sd=P["sd"] + 2), q(color=None), q(color=P["col"] + 8),
        q(c=P["c"] + 1), q(so=P["so"] + 2), q(cnt=P["n"] + 2),
        x(h=None), x(params=False), x(gbuffer=False), x(samples=0), x(samples=65), x(reserved=1), x(gp=None), x(gp=P["gp"] + 8), x(gn=None),
        x(gn=P["gn"] + 4), x(gd=None), x(gd=P["gd"] + 4), x(out=None), x(out=P["img"] + 8),
    ]
    assert all(rc == -1 for rc in bad), bad
    assert q(num=0, sf=None, sd=None, color=None) == 0
    torch.cuda.synchronize()
    for t in list(outs.values()) + [col, img]:
        assert (host(t) == -7).all()
    # and the good calls: every record at the origin with N = 0 has NdotL = 0, so colour 0 after its draws; a zero
    # worldPosition.w is the background, which takes the (zero) diffuse channel
    assert q(al=P["b"], c=P["c"], so=P["so"], cnt=P["n"]) == 0 and q() == 0 and x() == 0  # (no camera: the pass needs none)
    torch.cuda.synchronize()
    assert (host(col) == np.array([0, 0, 0, 1], F)).all() and (host(outs["c"]) == 0).all()
    assert (host(outs["so"]).view(U) == en.draws(np.zeros(1, U), 16)[1][0]).all()
    assert (host(img) == np.array([0, 0, 0, 1], F)).all()
    ctx.close()


def test_cpp_host_sky_equals_the_python_pipeline(pkg, tmp_path):
    """bdpt_render --env probe.hdr --sky 4 --raw on the Cornell box at 64 x 36, frame 0, equals FramePipeline.sky_lighting(4)
    under the same probe; without --env, or with --sky 0 / 65, bdpt_render refuses with a message"""
    import torch
    import __graft_entry__ as ge
    exe = os.path.join(ge.PKG_DIR, "host", "bdpt_render")
    assert os.path.exists(exe), "host/bdpt_render not built (run __graft_entry__.build())"
    w, h = 64, 36
    probe = tmp_path / "probe.hdr"
    env = _write_hdr(pkg, probe, 16, 8)
    raw = tmp_path / "sky.f32"
    r = subprocess.run([exe, "--scene", "cornell", "--width", str(w), "--height", str(h), "--frames", "1", "--env", str(probe), "--sky", "4",
                        "--out", str(tmp_path / "sky.pfm"), "--raw", str(raw)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    cpp = np.fromfile(raw, F).reshape(h, w, 4)
    scene = pkg.Scene.cornell()
    pipe = pkg.FramePipeline(scene, w, h)
    t = gpu(env)
    pipe.ctx.set_environment(t.data_ptr(), 16, 8)
    gp = pipe.gbuffer_params()
    gp.envMap, gp.envWidth, gp.envHeight = t.data_ptr(), 16, 8
    pipe.ctx.gbuffer_execute(gp, pipe.gb, pipe._stream_ptr())
    img = pipe.sky_lighting(4)
    torch.cuda.synchronize()
    assert pipe.last_sky_params.frameCount == 0
    assert np.array_equal(bits(cpp), bits(host(img)))
    assert (cpp[..., 3] == 1.0).all() and (cpp[..., 0:3] > 0).any()
    for args, text in ((["--sky", "4"], "--env"), (["--env", str(probe), "--sky", "0"], "--sky N"), (["--env", str(probe), "--sky", "65"], "--sky N"),
                       (["--sky-clamp", "2"], "goes with --sky")):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and text in r.stderr, (args, r.stderr)
    pipe.close()
    scene.close()


def _write_hdr(pkg, path, w, h):
    """a flat (uncompressed) Radiance .hdr of random RGBE texels -> the (h, w, 4) float32 map bdpt_image_load_hdr decodes it to"""
    rng = np.random.default_rng(6)
    rgbe = np.concatenate([rng.integers(1, 256, (h, w, 3)), rng.integers(126, 132, (h, w, 1))], axis=2).astype(np.uint8)
    rgbe[:, 0, 0] = 100  # (a row that starts 2, 2 would read as a run-length scanline)
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n" + f"-Y {h} +X {w}\n".encode() + rgbe.tobytes())
    lib = pkg.load_library()
    ww, hh, msg = C.c_uint32(), C.c_uint32(), C.create_string_buffer(256)
    env = np.zeros((h, w, 4), F)
    assert lib.bdpt_image_load_hdr(str(path).encode(), C.byref(ww), C.byref(hh), env.ctypes.data, env.size, msg, 256) == 0, msg.value
    assert (ww.value, hh.value) == (w, h) and (env[..., :3] > 0).all()
    return env
