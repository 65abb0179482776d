"""GPU tests of area lights (BDPT_PARAM_AREA_LIGHTS; contract: include/bdpt.h "Area lights").  The test scene is the
Cornell box with its emissive ceiling patch (a large constant emitter), a floating textured emitter and a floating
alpha-masked emitter, lit by nothing else: its one point light has intensity 0, so every point-light term is exactly +0."""
import ctypes as C
import math

import numpy as np
import pytest

from area_light_numpy import AREA_KEY
from area_scenes import AREA, EMISSIVE_HITS, MIS_POWER, NO_CONNECT, NO_NEE, NO_SPLAT, AreaScene
from hlsl_integrator_numpy import hm_init_rand
from hlsl_reference_math import next_rand

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def cornell(pkg):
    s = pkg.Scene.cornell()
    yield s
    s.close()


def _bits(t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _frame(pipe, flags, frame=None, gbuffer=True):
    import torch
    if frame is not None:
        pipe.gbuffer_frame, pipe.bdpt_frame = 0xdeadbeef + frame, 0x1337 + frame
    pipe.render_frame(extra_flags=flags, gbuffer=gbuffer)
    torch.cuda.synchronize()
    return pipe.output.clone()


def _means(pkg, scene, mat, depth, flags, frames):
    """per-pixel mean and sample variance of the frame's RGB luminance-free channels over `frames` frames (one G-buffer,
    no jitter)"""
    import torch
    pipe = pkg.FramePipeline(scene, 64, 64, max_depth=depth, mat_index=mat, clamp_upper=1e30)
    pipe.use_jitter = False
    st = pipe._stream_ptr()
    pipe.ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, st)
    s1 = torch.zeros(64, 64, 3, dtype=torch.float64, device=pipe.dev)
    s2 = torch.zeros_like(s1)
    out = pipe.output
    for k in range(frames):
        pipe.bdpt_frame = 0x1337 + k
        pipe.ctx.execute(pipe.bdpt_params(flags), pipe.gb, C.c_void_p(out.data_ptr()), st)
        v = out[..., :3].double()
        s1 += v
        s2 += v * v
    torch.cuda.synchronize()
    m = (s1 / frames).cpu().numpy()
    var = ((s2 - s1 * s1 / frames) / (frames - 1)).clamp_min(0).cpu().numpy()
    pipe.close()
    return m, var


@pytest.mark.parametrize("mat", [1, 0])
def test_nee_term0_agrees_with_emissive_hits(pkg, cornell, mat):
    """(1) NEE term 0 towards the emitters (A) and the emission the ray leaving eye vertex 1 finds (B) estimate the same
    one-bounce integral: they agree in every 8x8 block within 5 standard errors and in the global mean within 2 %."""
    scene = AreaScene(pkg, cornell)
    frames = 10000
    mA, vA = _means(pkg, scene, mat, 1, AREA | NO_SPLAT | NO_CONNECT, frames)
    mB, vB = _means(pkg, scene, mat, 2, EMISSIVE_HITS | NO_NEE | NO_SPLAT | NO_CONNECT, frames)
    blk = lambda x: x.reshape(8, 8, 8, 8, 3).sum(axis=(1, 3))
    bA, bB = blk(mA) / 64, blk(mB) / 64
    se = np.sqrt(blk(vA) / frames + blk(vB) / frames) / 64
    z = np.abs(bA - bB) / np.maximum(se, 1e-30)
    # (a block that differs by less than 1e-4 of the frame's mean agrees too: there B can find emission only at grazing
    # angles, a rare event that 1e4 cosine samples may miss altogether, so its sample variance says nothing)
    ok = (np.abs(bA - bB) <= 5 * se) | (np.abs(bA - bB) <= 1e-4 * mB.mean())
    w = np.unravel_index(np.argmax(z), z.shape)
    assert ok.all(), f"worst block z = {z.max():.2f} at {w}: A {bA[w]:.6g} B {bB[w]:.6g} se {se[w]:.3g}; means {mA.mean():.6g} {mB.mean():.6g}"
    gA, gB = mA.mean(), mB.mean()
    assert gA > 0 and abs(gA - gB) <= 0.02 * gB, (gA, gB)
    # without the switch frame A is the G-buffer emission alone (the point light is dark): the test fails without the feature
    m0, _ = _means(pkg, scene, mat, 1, NO_SPLAT | NO_CONNECT, 4)
    assert gA - m0.mean() > 0.05 * gA


def test_sampler_matches_numpy_restatement(pkg, cornell):
    """(2) the hook's samples against area_light_numpy: prim (except within 1e-6 of a CDF boundary), position, direction,
    colour and NEE intensity within 1e-4 relative; prim frequencies against w_i / W by chi-squared over 1e6 samples."""
    scene = AreaScene(pkg, cornell)
    ctx = pkg.Context(0)
    ctx.set_scene(scene.desc)
    info = ctx.area_light_info()
    tab = scene.table()
    assert info.numEmitters == len(tab.prim) == 6 and info.numTextured == 2
    assert math.isclose(info.totalWeight, tab.W, rel_tol=1e-5)
    rng = np.random.default_rng(5)
    n = 4000
    states = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    out0 = ctx.test_area_light_sample(0, states)
    pts = np.stack([rng.uniform(0, 555, n), rng.uniform(0, 540, n), rng.uniform(0, 555, n)], 1).astype(np.float32)
    out1 = ctx.test_area_light_sample(1, states, pts)
    u32 = lambda x: x.view(np.uint32)
    checked = 0
    for k in range(n):
        s, a = next_rand(int(states[k]))
        near = np.min(np.abs(tab.cdf - a * tab.W)) <= 1e-6 * tab.W
        x, nrm, dirv, col, seed = tab.light_start(int(states[k]))
        if near or (x["alpha"] is not None and abs(x["alpha"][0] - x["alpha"][1]) < 1e-4):
            continue
        checked += 1
        g = out0[k]
        assert int(u32(g[0:1])[0]) == x["prim"], k
        assert np.allclose(g[1:3], [x["b1"], x["b2"]], rtol=1e-4, atol=1e-5)
        assert np.allclose(g[3:6], x["pos"], rtol=1e-4, atol=1e-3)
        assert np.allclose(g[6:9], nrm, atol=1e-5)
        assert np.allclose(g[9:12], dirv, atol=2e-4)
        assert np.allclose(g[12:15], col, rtol=1e-4, atol=1e-6 * max(1.0, float(np.abs(col).max())))
        assert int(u32(g[15:16])[0]) == seed
        xn, L, d, inten = tab.nee(int(states[k]), pts[k].astype(np.float64))
        h = out1[k]
        _, an = next_rand(hm_init_rand(int(states[k]), AREA_KEY))
        if np.min(np.abs(tab.cdf - an * tab.W)) <= 1e-6 * tab.W or (
                xn["alpha"] is not None and abs(xn["alpha"][0] - xn["alpha"][1]) < 1e-4):
            continue
        assert int(u32(h[0:1])[0]) == xn["prim"], k
        if d < 5.0:
            continue  # (fp32 positions of a 555-unit box put ~3e-5 into x - pos: within 5 units that exceeds 1e-4 of d^2)
        assert np.allclose(h[1:4], L, atol=1e-4) and math.isclose(h[4], d, rel_tol=1e-4)
        # (at grazing emission |dot(n_g, L)| is small and its fp32 rounding dominates: allow 1e-5 of the cos = 1 value)
        scale = float(np.abs(xn["Le"]).max()) / (xn["pA"] * d * d)
        assert np.allclose(h[5:8], inten, rtol=1e-4, atol=1e-5 * scale), k
    assert checked > 0.95 * n
    # chi-squared of prim frequencies over 1e6 NEE samples
    big = rng.integers(0, 2**32, 1000000, dtype=np.uint64).astype(np.uint32)
    o = ctx.test_area_light_sample(1, big, np.zeros((len(big), 3), np.float32))
    prims = u32(o[:, 0].copy())
    counts = np.array([(prims == p).sum() for p in tab.prim], np.float64)
    expect = tab.w / tab.W * len(big)
    chi2 = float(((counts - expect) ** 2 / np.maximum(expect, 1e-9)).sum())
    assert counts.sum() == len(big) and chi2 < 40.0, (chi2, counts, expect)  # 5 degrees of freedom: p ~ 1e-7
    ctx.close()


def test_no_emitters_switch_is_a_no_op(pkg, cornell):
    """(3) the Cornell box with material 3's emission zeroed has no emitter: frames with and without the switch are
    bit-identical (both matrices, and with EMISSIVE_HITS)."""
    scene = AreaScene(pkg, cornell, patch_emission=(0.0, 0.0, 0.0), extra=False)
    for mat in (0, 1):
        pipe = pkg.FramePipeline(scene, 96, 64, max_depth=5, mat_index=mat)
        assert pipe.ctx.area_light_info().numEmitters == 0
        for extra in (0, EMISSIVE_HITS):
            a = _frame(pipe, extra, frame=0)
            b = _frame(pipe, extra | AREA, frame=0)
            assert np.array_equal(_bits(a), _bits(b)), (mat, extra)
        pipe.close()


def _area_pipe(pkg, scene, W=96, H=64, D=5, mat=0, **kw):
    return pkg.FramePipeline(scene, W, H, max_depth=D, mat_index=mat, **kw)


def test_masked_frames_equal_execute_on_active_pixels(pkg, cornell):
    """(4) with the switch, an all-ones mask and a random mask give bdpt_execute's bits on the active pixels."""
    import torch
    scene = AreaScene(pkg, cornell)
    pipe = _area_pipe(pkg, scene)
    ref = _frame(pipe, AREA, frame=3)
    plain = _frame(pipe, 0, frame=3)
    assert not np.array_equal(_bits(ref), _bits(plain))  # the switch is live
    rng = np.random.default_rng(2)
    for mask_np in (np.ones((64, 96), np.uint8), (rng.random((64, 96)) < 0.4).astype(np.uint8)):
        mask = torch.from_numpy(mask_np).cuda()
        out = torch.full((64, 96, 4), 7.0, dtype=torch.float32, device="cuda")
        pipe.gbuffer_frame, pipe.bdpt_frame = 0xdeadbeef + 3, 0x1337 + 3
        st = pipe._stream_ptr()
        pipe.ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, st)
        pipe.ctx.execute_masked(pipe.bdpt_params(AREA), pipe.gb, C.c_void_p(mask.data_ptr()), C.c_void_p(out.data_ptr()), st)
        torch.cuda.synchronize()
        on = mask_np != 0
        assert np.array_equal(_bits(out)[on], _bits(ref)[on])
        assert (out.cpu().numpy()[~on] == 7.0).all()
    pipe.close()


@pytest.mark.parametrize("world", [2, 4])
def test_stripes_reassemble_whole_frame(pkg, cornell, world):
    """(5) 2 and 4 striped contexts with the switch reassemble to the whole-frame image bit for bit."""
    from test_gpu_configs import _stripes_equal_full
    scene = AreaScene(pkg, cornell)
    _stripes_equal_full(pkg, scene, 64, 45, 5, 0, world, flags=AREA)


def test_refit_equals_fresh_context(pkg, cornell):
    """(6) the Cornell patch moved and scaled by bdpt_update_geometry renders the frame of a fresh context on the moved
    scene, bit for bit; totalWeight follows the new area."""
    import torch
    scene = AreaScene(pkg, cornell)
    pipe = _area_pipe(pkg, scene)
    w0 = pipe.ctx.area_light_info().totalWeight
    _frame(pipe, AREA, frame=0)
    P = scene.P.copy()
    patch = np.unique(scene.I[scene.M == 3])
    c = P[patch].mean(axis=0)
    P[patch] = (P[patch] - c) * np.array([1.5, 1.0, 1.5], np.float32) + c + np.array([30.0, -20.0, 10.0], np.float32)
    pipe.update_geometry(torch.from_numpy(np.ascontiguousarray(P)).cuda())
    got = _frame(pipe, AREA, frame=1)
    moved = AreaScene(pkg, cornell, positions=P[: cornell.desc.numVertices])
    fresh = _area_pipe(pkg, moved)
    want = _frame(fresh, AREA, frame=1)
    assert np.array_equal(_bits(got), _bits(want))
    w1 = pipe.ctx.area_light_info().totalWeight
    assert math.isclose(w1, fresh.ctx.area_light_info().totalWeight, rel_tol=0, abs_tol=0)
    tab = scene.table()
    patch_w = tab.w[np.isin(tab.prim, np.nonzero(scene.M == 3)[0])].sum()
    assert math.isclose(w1 - w0, patch_w * (2.25 - 1.0), rel_tol=1e-4)
    pipe.close()
    fresh.close()


def test_update_and_switched_frame_captured_in_a_hip_graph(pkg, cornell):
    """(7) after bdpt_prepare(AREA_LIGHTS | REFIT | PRIMARY) an update plus a switched frame captured in a graph replays
    bit-exact."""
    import torch
    scene = AreaScene(pkg, cornell)
    pipe = _area_pipe(pkg, scene)
    pipe.ctx.prepare(pkg.abi.PREPARE_AREA_LIGHTS | pkg.abi.PREPARE_REFIT | pkg.abi.PREPARE_PRIMARY)
    P1 = scene.P.copy()
    P1[np.unique(scene.I[scene.M == 3])] += np.array([20.0, 0.0, -15.0], np.float32)
    p1 = torch.from_numpy(np.ascontiguousarray(P1)).cuda()
    p0 = torch.from_numpy(np.ascontiguousarray(scene.P)).cuda()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        pipe.update_geometry(p1)
        pipe.render_frame(extra_flags=AREA)
    torch.cuda.synchronize()
    ref = pipe.output.clone()
    pipe.gbuffer_frame, pipe.bdpt_frame = 0xdeadbeef, 0x1337
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        pipe.update_geometry(p0)
        graph.capture_begin()
        pipe.update_geometry(p1)
        pipe.render_frame(extra_flags=AREA)
        graph.capture_end()
    torch.cuda.synchronize()
    for _ in range(2):
        pipe.output.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(pipe.output, ref)
    del graph
    pipe.close()


def test_errors_and_determinism(pkg, cornell):
    """(8) the switch with MIS or with light groups is BDPT_E_INVALID with a message; two runs of a frame are identical."""
    import torch
    scene = AreaScene(pkg, cornell)
    pipe = _area_pipe(pkg, scene, light_groups=False)
    lib = pkg.load_library()
    st = pipe._stream_ptr()
    pipe.ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, st)
    out = pipe.output
    for bad in (MIS_POWER, 128):
        rc = lib.bdpt_execute(pipe.ctx._h, C.byref(pipe.bdpt_params(AREA | bad)), C.byref(pipe.gb), C.c_void_p(out.data_ptr()), st)
        assert rc == -1 and b"AREA_LIGHTS" in lib.bdpt_last_error(pipe.ctx._h)
    groups = torch.zeros(2, 64, 96, 4, dtype=torch.float32, device="cuda")
    rc = lib.bdpt_execute_light_groups(pipe.ctx._h, C.byref(pipe.bdpt_params(AREA)), C.byref(pipe.gb), C.c_void_p(out.data_ptr()),
                                       C.c_void_p(groups.data_ptr()), st)
    assert rc == -1 and b"AREA_LIGHTS" in lib.bdpt_last_error(pipe.ctx._h)
    a = _frame(pipe, AREA, frame=5)
    b = _frame(pipe, AREA, frame=5)
    assert np.array_equal(_bits(a), _bits(b))
    assert np.isfinite(a.cpu().numpy()).all()
    pipe.close()


def test_cpp_host_area_lights_flag(pkg, tmp_path):
    """(9) bdpt_render --area-lights on the Cornell box writes a frame that differs from the run without it, with no NaN
    or Inf."""
    import os
    import subprocess
    import __graft_entry__ as ge
    exe = os.path.join(ge.PKG_DIR, "host", "bdpt_render")
    assert os.path.exists(exe), "host/bdpt_render not built (run __graft_entry__.build())"
    W, H = 96, 64
    imgs = []
    for extra in ([], ["--area-lights"]):
        raw = tmp_path / f"out{len(extra)}.f32"
        r = subprocess.run([exe, "--scene", "cornell", "--width", str(W), "--height", str(H), "--frames", "3", "--depth", "4",
                            "--out", str(tmp_path / f"o{len(extra)}.pfm"), "--raw", str(raw)] + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        imgs.append(np.fromfile(raw, np.float32).reshape(H, W, 4))
    assert np.isfinite(imgs[1]).all()
    assert not np.array_equal(imgs[0], imgs[1])
