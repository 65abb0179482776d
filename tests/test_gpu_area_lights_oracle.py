"""GPU frames and the sampling hook with area lights (BDPT_PARAM_AREA_LIGHTS) against the CPU oracle, bit for bit: G-buffer
channels, the u64 splat buffer and the resolved image of whole-frame, band, deferred, masked and refitted contexts, and
every float of bdpt_test_area_light_sample on tables of up to ~70 000 emitters."""
import ctypes as C

import numpy as np
import pytest

from area_scenes import (AREA, DEFER_RESOLVE, DEFER_TAIL, EMISSIVE_HITS, ENV_ON_MISS, NEE_TOP_DRAW_STATES, NO_CONNECT, NO_NEE,
                         NO_SPLAT, AreaScene, DescArrays, bits, copy_desc, emitter_soup, oracle_exclude, oracle_info,
                         oracle_sample, states_for_top_draw)

pytestmark = pytest.mark.gpu

CHANNELS = {"WorldPosition": "worldPosition", "WorldNormal": "worldNormal", "MaterialDiffuse": "materialDiffuse",
            "MaterialSpecRough": "materialSpecRough", "MaterialExtraParams": "materialExtra", "Emissive": "emissive"}
ENV = (0.3, 0.45, 0.7, 1.0)


@pytest.fixture(scope="module")
def cornell(pkg):
    s = pkg.Scene.cornell()
    yield s
    s.close()


def _splat(pipe):
    import torch
    ptr, n64 = pipe.ctx.splat_buffer()
    spl = torch.empty(n64, dtype=torch.int64, device=pipe.dev)
    torch.cuda.synchronize()
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(C.c_void_p(spl.data_ptr()), C.c_void_p(ptr), C.c_size_t(n64 * 8), 3) == 0
    return spl.cpu().numpy().view(np.uint64).reshape(-1, 4)


def _oracle(pkg, ob, scene, pipe, gp, p, dropped=()):
    orc = ob.OracleRender(pkg.abi, scene.desc, pipe.W, pipe.H, pipe.y0, pipe.y1)
    if len(dropped):
        oracle_exclude(orc.lib, orc.scene, dropped)
    orc.set_environment(None, ENV)
    orc.gbuffer(pipe.cam, gp)
    cnt = orc.bdpt(pipe.cam, p)
    return orc, cnt


def _check_info(pkg, ob, pipe, scene, dropped=()):
    lib = ob.load_oracle(pkg.abi)
    osc = lib.oracle_scene_create(C.byref(scene.desc))
    if len(dropped):
        oracle_exclude(lib, osc, dropped)
    o, g = oracle_info(pkg, lib, osc), pipe.ctx.area_light_info()
    lib.oracle_scene_destroy(osc)
    assert (g.numEmitters, g.numTextured) == (o.numEmitters, o.numTextured) and bits([g.totalWeight]) == bits([o.totalWeight])
    assert g.numEmitters > 0 and g.totalWeight > 0
    return g


def _frames_match(pkg, ob, scene, pipe, flags, frames=2, dropped=()):
    """`frames` frames with the switch: channels, splat buffer and resolved image equal the oracle's bit for bit (the
    context's rows); the ray and pixel counters relate as in test_atrium_frame_matches_oracle"""
    import torch
    pipe.ctx.set_environment(None, 0, 0, ENV)
    y0, y1 = pipe.y0, pipe.y1
    for k in range(frames):
        gp, p = pipe.render_frame(extra_flags=flags | AREA)
        torch.cuda.synchronize()
        orc, cnt = _oracle(pkg, ob, scene, pipe, gp, p, dropped)
        for ch, on in CHANNELS.items():
            g = pipe.channels[ch].float().cpu().numpy().reshape(pipe.H, pipe.W, 4)[y0:y1]
            assert np.array_equal(bits(g), bits(orc.chan[on].reshape(pipe.H, pipe.W, 4)[y0:y1])), (ch, k)
        assert np.array_equal(_splat(pipe), orc.splat), ("splat", k, flags)
        orc.resolve()
        gpu = pipe.output.cpu().numpy()[y0:y1]
        ref = orc.image()[y0:y1]
        assert np.array_equal(bits(gpu), bits(ref)), f"frame {k} flags {flags}: {(bits(gpu) != bits(ref)).any(axis=-1).sum()} pixels differ"
        c, o = pipe.ctx.counters().as_dict(), cnt.as_dict()
        assert c["raysEyeExtend"] == o["raysEyeExtend"] and c["raysLightExtend"] == o["raysLightExtend"]
        assert c["raysSplat"] <= o["raysSplat"] and c["raysNee"] <= o["raysNee"] and c["raysConnect"] <= o["raysConnect"]
        assert c["pixelsValid"] == o["pixelsValid"] and c["splatsLanded"] == o["splatsLanded"]
        orc.close()


# (mat, depth, flags, relit): every depth of 1, 2, 5, 8; each flag with both materials at a depth of at least 5
MATRIX = [(0, 1, 0, False), (1, 2, 0, True), (0, 5, 0, True), (1, 8, 0, False),
          (0, 5, NO_NEE, False), (1, 8, NO_NEE, True),
          (1, 5, NO_SPLAT, False), (0, 8, NO_SPLAT, True),
          (0, 8, NO_CONNECT, False), (1, 5, NO_CONNECT, True),
          (0, 5, EMISSIVE_HITS, True), (1, 5, EMISSIVE_HITS, False),
          (1, 8, ENV_ON_MISS, True), (0, 5, ENV_ON_MISS | EMISSIVE_HITS, False), (0, 2, ENV_ON_MISS, False)]


@pytest.mark.parametrize("mat,depth,flags,relit", MATRIX)
def test_cornell_area_frames_match_oracle(pkg, ob, cornell, mat, depth, flags, relit):
    """The Cornell AreaScene (ceiling patch, textured and alpha-masked emitters) with its point light on; `relit` adds a
    spot, a second point and a directional light: point lights and the table share the numLights + 1 choice."""
    scene = AreaScene(pkg, cornell, point_light=True, relit=relit)
    pipe = pkg.FramePipeline(scene, 48, 40, max_depth=depth, mat_index=mat)
    _check_info(pkg, ob, pipe, scene)
    _frames_match(pkg, ob, scene, pipe, flags)
    pipe.close()


def test_atrium_area_frame_matches_oracle(pkg, ob):
    """The atrium: its lamp bodies are the emitters; 96x54, depth 5, GGX."""
    scene = pkg.Scene.atrium(1, 30000)
    pipe = pkg.FramePipeline(scene, 96, 54, max_depth=5, mat_index=0)
    assert _check_info(pkg, ob, pipe, scene).numEmitters >= 2
    _frames_match(pkg, ob, scene, pipe, 0, frames=1)
    pipe.close()
    scene.close()


def test_table_with_zero_total_weight_changes_nothing(pkg, ob, cornell):
    """A table whose emitters all have zero area (W == 0): the frame with the switch is the frame without it, bit for bit,
    on the device and in the oracle, and both equal each other."""
    import torch
    scene = AreaScene(pkg, cornell, point_light=True, relit=True, extra=False)
    patch = np.unique(scene.I[scene.M == 3])
    P = scene.P.copy()
    P[patch] = P[patch[0]]  # every corner of the ceiling patch on one point
    flat = AreaScene(pkg, cornell, point_light=True, relit=True, extra=False, positions=P)
    pipe = pkg.FramePipeline(flat, 48, 40, max_depth=5, mat_index=0)
    info = pipe.ctx.area_light_info()
    assert info.numEmitters == len(flat.table().prim) > 0 and info.totalWeight == 0.0
    pipe.ctx.set_environment(None, 0, 0, ENV)
    imgs = []
    for flags in (AREA, 0):
        pipe.gbuffer_frame, pipe.bdpt_frame = 0xdeadbeef, 0x1337
        gp, p = pipe.render_frame(extra_flags=flags | EMISSIVE_HITS)
        torch.cuda.synchronize()
        imgs.append((bits(pipe.output).copy(), _splat(pipe).copy()))
        orc, _ = _oracle(pkg, ob, flat, pipe, gp, p)
        assert oracle_info(pkg, orc.lib, orc.scene).totalWeight == 0.0
        assert np.array_equal(_splat(pipe), orc.splat)
        orc.resolve()
        assert np.array_equal(imgs[-1][0], bits(orc.image()))
        orc.close()
    assert np.array_equal(imgs[0][0], imgs[1][0]) and np.array_equal(imgs[0][1], imgs[1][1])
    pipe.close()


def _courtyard_with_emitters(pkg, base):
    """The foliage courtyard with every 7th opaque triangle emissive and two fully transparent emissive cards (dropped by
    the build); returns (scene, the cards' triangles)"""
    a = pkg.abi
    c = copy_desc(pkg, base.desc)
    P, N, T, B, I, M, mats, textures = (c[k] for k in ("P", "N", "T", "B", "I", "M", "mats", "textures"))
    nt = I.shape[0]
    opaque = [t for t in range(nt) if ((mats[M[t]].flags >> 17) & 3) == 0]
    for t in opaque[::7]:
        m = a.Material()
        C.memmove(C.byref(m), C.byref(mats[M[t]]), C.sizeof(a.Material))
        m.flags = (m.flags & ~(7 << 9)) | (1 << 9)
        m.emissive[:] = (1.5, 1.2, 0.8)
        mats.append(m)
        M[t] = len(mats) - 1
    tex_t = np.full((2, 2, 4), 90, np.uint8)
    tex_t[..., 3] = 0
    textures.append((tex_t, False))
    card = a.Material()
    C.memmove(C.byref(card), C.byref(mats[0]), C.sizeof(a.Material))
    card.flags = (1 << 17) | (2 << 3) | (1 << 9)  # alpha mask, diffuse from the texture, constant emission
    card.texBaseColor, card.texEmissive, card.texNormal, card.texSpecular = len(textures) - 1, -1, -1, -1
    card.alphaThreshold = 0.5
    card.emissive[:] = (5.0, 5.0, 5.0)
    mats.append(card)
    dropped = []
    centre = P.mean(axis=0)
    for k in range(2):
        q = (centre + np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32) * 2.0 + np.float32(k * 3)).astype(np.float32)
        dropped += [I.shape[0], I.shape[0] + 1]
        I = np.concatenate([I, np.array([[0, 1, 2], [0, 2, 3]], np.uint32) + P.shape[0]])
        P = np.concatenate([P, q])
        N = np.concatenate([N, np.tile([[0, 0, 1]], (4, 1)).astype(np.float32)])
        T = np.concatenate([T, np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)])
        if B is not None:
            B = np.concatenate([B, np.tile([[0, 1, 0]], (4, 1)).astype(np.float32)])
        M = np.concatenate([M, np.array([len(mats) - 1] * 2, np.uint32)])
    sc = DescArrays(a, P, N, T, I, M, mats, textures, c["lights"], B=B)
    sc.camera = base.camera
    return sc, dropped


def test_courtyard_with_dropped_emitters_matches_oracle(pkg, ob):
    """The foliage courtyard with emission on some non-foliage triangles and fully transparent emissive cards: the table
    goes through the marking of the triangles the tree references (numDropped > 0); the oracle is told which emitters
    were dropped (oracle_area_exclude)."""
    base = pkg.Scene.courtyard(5, 7000, 0.35)
    ref_ctx = pkg.Context(0)
    ref_ctx.set_scene(base.desc)
    dropped0 = ref_ctx.bvh_info().numDropped
    ref_ctx.close()
    scene, cards = _courtyard_with_emitters(pkg, base)
    pipe = pkg.FramePipeline(scene, 64, 40, max_depth=5, mat_index=0)
    assert pipe.ctx.bvh_info().numDropped == dropped0 + len(cards) > 0
    _check_info(pkg, ob, pipe, scene, dropped=cards)
    _frames_match(pkg, ob, scene, pipe, 0, frames=1, dropped=cards)
    pipe.close()
    base.close()


def test_transparent_emissive_quad_is_dropped_and_excluded(pkg, ob, cornell):
    """A fully transparent alpha-masked emissive quad in the box: the build drops both triangles, the table leaves them
    out, and the oracle told so (oracle_area_exclude) renders the same frames."""
    scene = AreaScene(pkg, cornell, point_light=True, transparent=True)
    pipe = pkg.FramePipeline(scene, 48, 40, max_depth=5, mat_index=1)
    assert pipe.ctx.bvh_info().numDropped == len(scene.dropped) == 2
    g = _check_info(pkg, ob, pipe, scene, dropped=scene.dropped)
    assert g.numEmitters == len(scene.table(dropped=scene.dropped).prim) == len(scene.table().prim) - 2
    _frames_match(pkg, ob, scene, pipe, 0, dropped=scene.dropped)
    pipe.close()


def test_band_deferred_masked_and_refit_contexts_match_oracle(pkg, ob, cornell):
    """A band context tile=(y0, y1); DEFER_RESOLVE (own-pixel terms + splat buffer) and DEFER_TAIL (+ execute_tail); a
    masked frame on its active pixels; and a context after bdpt_update_geometry against the oracle of the moved scene."""
    import torch
    scene = AreaScene(pkg, cornell, point_light=True, relit=True)
    W, H, D = 48, 40, 5
    band = pkg.FramePipeline(scene, W, H, max_depth=D, mat_index=0, tile=(13, 29))
    _frames_match(pkg, ob, scene, band, 0, frames=1)
    band.close()
    pipe = pkg.FramePipeline(scene, W, H, max_depth=D, mat_index=1)
    pipe.ctx.set_environment(None, 0, 0, ENV)
    # DEFER_RESOLVE: the output holds the own-pixel terms, the splat buffer the rest
    gp, p = pipe.render_frame(extra_flags=AREA | DEFER_RESOLVE)
    torch.cuda.synchronize()
    orc, _ = _oracle(pkg, ob, scene, pipe, gp, p)
    assert np.array_equal(_splat(pipe), orc.splat)
    assert np.array_equal(bits(pipe.output), bits(orc.image()))
    orc.close()
    # DEFER_TAIL: execute_tail enqueues the rest and resolves
    gp, p = pipe.render_frame(extra_flags=AREA | DEFER_TAIL)
    pipe.ctx.execute_tail(p, pipe.gb, C.c_void_p(pipe.output.data_ptr()), pipe._stream_ptr())
    torch.cuda.synchronize()
    orc, _ = _oracle(pkg, ob, scene, pipe, gp, p)
    assert np.array_equal(_splat(pipe), orc.splat)
    orc.resolve()
    assert np.array_equal(bits(pipe.output), bits(orc.image()))
    orc.close()
    # masked frame: the active pixels
    mask_np = (np.random.default_rng(4).random((H, W)) < 0.5).astype(np.uint8)
    mask = torch.from_numpy(mask_np).cuda()
    out = torch.full((H, W, 4), 7.0, dtype=torch.float32, device="cuda")
    gp, p = pipe.gbuffer_params(), pipe.bdpt_params(AREA)
    st = pipe._stream_ptr()
    pipe.ctx.gbuffer_execute(gp, pipe.gb, st)
    pipe.ctx.execute_masked(p, pipe.gb, C.c_void_p(mask.data_ptr()), C.c_void_p(out.data_ptr()), st)
    torch.cuda.synchronize()
    orc, _ = _oracle(pkg, ob, scene, pipe, gp, p)
    orc.resolve()
    on = mask_np != 0
    assert np.array_equal(bits(out)[on], bits(orc.image())[on]) and (out.cpu().numpy()[~on] == 7.0).all()
    orc.close()
    # after an update that moves and scales the ceiling patch and the textured emitter
    P = scene.P.copy()
    for mid in (3, int(scene.M[-4])):
        idx = np.unique(scene.I[scene.M == mid])
        c = P[idx].mean(axis=0)
        P[idx] = (P[idx] - c) * np.array([1.5, 1.0, 1.25], np.float32) + c + np.array([25.0, -15.0, 10.0], np.float32)
    pipe.update_geometry(torch.from_numpy(np.ascontiguousarray(P)).cuda())
    moved = AreaScene(pkg, cornell, point_light=True, relit=True, positions=P)
    assert np.array_equal(moved.P, P)
    _check_info(pkg, ob, pipe, moved)
    _frames_match(pkg, ob, moved, pipe, 0, frames=1)
    pipe.close()


def _hook_matches(pkg, ob, ctx, desc, states, pts, chunk=1 << 18):
    lib = ob.load_oracle(pkg.abi)
    osc = lib.oracle_scene_create(C.byref(desc))
    o, g = oracle_info(pkg, lib, osc), ctx.area_light_info()
    assert (g.numEmitters, g.numTextured) == (o.numEmitters, o.numTextured) and bits([g.totalWeight]) == bits([o.totalWeight])
    for mode in (0, 1):
        for s0 in range(0, len(states), chunk):
            st = states[s0:s0 + chunk]
            pp = pts[s0:s0 + chunk] if mode == 1 else None
            dev = ctx.test_area_light_sample(mode, st, pp)
            ref = oracle_sample(lib, osc, mode, st, pp)
            diff = (bits(dev) != bits(ref)).any(axis=1)
            assert not diff.any(), f"mode {mode}: {int(diff.sum())} of {len(st)} items differ, first {int(np.argmax(diff)) + s0}"
    lib.oracle_scene_destroy(osc)
    return g


@pytest.mark.parametrize("n", [64, 65, 4096, 4097, 70000])
def test_area_hook_bit_exact_on_large_tables(pkg, ob, n):
    """bdpt_test_area_light_sample against oracle_area_light_sample, modes 0 and 1, all 16 floats, nothing skipped, on
    tables that straddle the wave (64), the chunk of wave sums (4096) and many chunks (~70 000: 18 chunks, so the carry
    between chunks matters); non-emitters and zero-luminance triangles interleaved; zero-area emitters and a run of them
    at the end; a 5x3 emission texture with wrapping UVs.  Random states plus states whose draw a is the largest below 1,
    for the light start and for the NEE stream.  Then again after an update that rescales every area."""
    sc = emitter_soup(pkg, n, seed=n + 1)
    ctx = pkg.Context(0)
    ctx.set_scene(sc.desc)
    rng = np.random.default_rng(n)
    k = 1_000_000 if n == 70000 else 50_000
    # random states, then light-start states whose a is the largest below 1 and NEE states whose AREA-stream a is
    states = np.concatenate([rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32), states_for_top_draw(4096, n),
                             NEE_TOP_DRAW_STATES])
    pts = rng.uniform(-5.0, 105.0, (len(states), 3)).astype(np.float32)
    g = _hook_matches(pkg, ob, ctx, sc.desc, states, pts)
    assert g.numEmitters >= n
    P2 = (sc.P * np.float32(1.7) - np.float32(3.0)).astype(np.float32)
    ctx.update_geometry(P2)
    moved = DescArrays(pkg.abi, P2, sc.N, sc.T, sc.I, sc.M, list(sc.mats), sc.textures, list(sc.lights))
    keep = np.r_[0:min(k, 200_000), k:len(states)]  # (and every top-draw state)
    g2 = _hook_matches(pkg, ob, ctx, moved.desc, states[keep], pts[keep])
    assert g2.totalWeight > 2.5 * g.totalWeight
    ctx.close()


def test_cpp_host_area_lights_matches_python_pipeline(pkg, ob, cornell, tmp_path):
    """bdpt_render --area-lights accumulates the image of the same frame sequence driven from Python with the switch, and
    its first frame is the oracle's."""
    import os
    import subprocess
    import torch
    import __graft_entry__ as ge
    exe = os.path.join(ge.PKG_DIR, "host", "bdpt_render")
    assert os.path.exists(exe), "host/bdpt_render not built (run __graft_entry__.build())"
    raw = tmp_path / "out.f32"
    size, frames = 48, 3

    def run(n):
        r = subprocess.run([exe, "--scene", "cornell", "--width", str(size), "--height", str(size), "--frames", str(n),
                            "--depth", "4", "--mat", "0", "--area-lights", "--out", str(tmp_path / "o.pfm"), "--raw", str(raw)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return np.fromfile(raw, np.float32).reshape(size, size, 4)
    cpp = run(frames)
    pipe = pkg.FramePipeline(cornell, size, size, max_depth=4, mat_index=0, accum_limit=100)
    first = None
    for k in range(frames):
        gp, p = pipe.render_frame(accumulate=True, extra_flags=AREA)
        if k == 0:
            first = (gp, p)
    torch.cuda.synchronize()
    assert np.array_equal(bits(cpp), bits(pipe.output))
    assert pipe.ctx.area_light_info().numEmitters > 0
    cpp1 = run(1)
    orc = ob.OracleRender(pkg.abi, cornell.desc, size, size)
    orc.gbuffer(pipe.cam, first[0])
    orc.bdpt(pipe.cam, first[1])
    orc.resolve()
    assert np.array_equal(bits(cpp1), bits(orc.image()))
    orc.close()
    pipe.close()
