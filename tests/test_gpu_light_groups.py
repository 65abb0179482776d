"""GPU tests of bdpt_execute_light_groups (contract: include/bdpt.h "Light groups").  Every comparison is bit for bit unless
stated: `out` against bdpt_execute's, the emission plane against the frame with every light's intensity zero, light
plane k's RGB against the frame with only light k, the G-buffer emissive and background zeroed and the walk's extra terms
off (the "stripped" frame), rendered by the same library on the same G-buffer, and once by the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RAY_KEYS = ("raysPrimary", "raysEyeExtend", "raysLightExtend", "raysNee", "raysSplat", "raysConnect", "pixelsValid",
            "splatsLanded", "raysConnectLazy", "hintedNee", "hintedSplat")
EXT = 1024 | 2048  # BDPT_PARAM_ENV_ON_MISS | BDPT_PARAM_EMISSIVE_HITS


def _bits(t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_bits(a, b, label):
    x, y = _bits(a), _bits(b)
    assert x.shape == y.shape, label
    if not np.array_equal(x, y):
        bad = (x != y).reshape(-1, x.shape[-1]).any(axis=-1).sum()
        raise AssertionError(f"{label}: {bad} pixels differ")


def _copy_lights(pkg, desc):
    out = [pkg.abi.Light() for _ in range(desc.numLights)]
    for i in range(desc.numLights):
        C.memmove(C.byref(out[i]), C.byref(desc.lights[i]), C.sizeof(pkg.abi.Light))
    return out


def _only(pkg, lights, k):
    """The lights with every intensity but light k's zero (k = None: all zero)."""
    out = []
    for i, l in enumerate(lights):
        m = pkg.abi.Light()
        C.memmove(C.byref(m), C.byref(l), C.sizeof(pkg.abi.Light))
        if i != k:
            m.intensity[0] = m.intensity[1] = m.intensity[2] = 0.0
        out.append(m)
    return out


class Frame:
    """One pipeline's G-buffer of one frame and the renders the tests compare, all with the same params."""

    def __init__(self, pkg, pipe, flags=0):
        import torch
        self.pkg, self.pipe, self.torch = pkg, pipe, torch
        st = pipe._stream_ptr()
        self.gp = pipe.gbuffer_params()
        pipe.ctx.gbuffer_execute(self.gp, pipe.gb, st)
        self.p = pipe.bdpt_params(flags)
        self.K = int(pipe.scene.desc.numLights)
        ch = pipe.channels
        # the stripped G-buffer: emissive RGB zero, background pixels' diffuse RGB zero
        self.em0 = ch["Emissive"].clone()
        self.em0[..., :3] = 0
        self.dif0 = ch["MaterialDiffuse"].clone()
        bg = ch["WorldPosition"][..., 3] == 0
        self.dif0[..., :3][bg] = 0
        names = ["WorldPosition", "WorldNormal", "MaterialDiffuse", "MaterialSpecRough", "MaterialExtraParams", "Emissive"]
        t = {n: ch[n] for n in names}
        t["MaterialDiffuse"], t["Emissive"] = self.dif0, self.em0
        self.gb0 = pkg.abi.GBuffer(*[t[n].data_ptr() for n in names])
        torch.cuda.synchronize()

    def _new(self, planes=None):
        shape = (self.pipe.H, self.pipe.W, 4) if planes is None else (planes, self.pipe.H, self.pipe.W, 4)
        return self.torch.full(shape, 7.0, dtype=self.torch.float32, device=self.pipe.dev)  # (a value no frame writes)

    def plain(self, params=None, gb=None):
        out = self._new()
        self.pipe.ctx.execute(params or self.p, gb or self.pipe.gb, C.c_void_p(out.data_ptr()), self.pipe._stream_ptr())
        self.torch.cuda.synchronize()
        return out, self.pipe.ctx.counters().as_dict()

    def groups(self):
        out, g = self._new(), self._new(self.K + 1)
        self.pipe.ctx.execute_light_groups(self.p, self.pipe.gb, C.c_void_p(out.data_ptr()), C.c_void_p(g.data_ptr()),
                                           self.pipe._stream_ptr())
        self.torch.cuda.synchronize()
        return out, g, self.pipe.ctx.counters().as_dict()

    def stripped(self, lights, k):
        """The frame light plane k must equal (RGB): only light k, stripped G-buffer, no ENV_ON_MISS / EMISSIVE_HITS."""
        p = self.pkg.abi.Params()
        C.pointer(p)[0] = self.p
        p.flags = self.p.flags & ~EXT
        self.pipe.ctx.set_lights(_only(self.pkg, lights, k), self.pipe._stream_ptr())
        out, _ = self.plain(p, self.gb0)
        self.pipe.ctx.set_lights(lights, self.pipe._stream_ptr())
        return out

    def emission(self, lights):
        """The frame the emission plane must equal (all four channels): every intensity zero, nothing else changed."""
        self.pipe.ctx.set_lights(_only(self.pkg, lights, None), self.pipe._stream_ptr())
        out, _ = self.plain()
        self.pipe.ctx.set_lights(lights, self.pipe._stream_ptr())
        return out


def _check_contract(pkg, pipe, flags, label, lights=None):
    """(1)-(3): out and counters equal bdpt_execute's, the emission plane the zero-intensity frame, each light plane's RGB
    the stripped frame, every plane's w out.w.  Returns (out, groups)."""
    lights = lights or _copy_lights(pkg, pipe.scene.desc)
    f = Frame(pkg, pipe, flags)
    ref, cref = f.plain()
    out, g, cg = f.groups()
    _assert_bits(out, ref, f"{label}: out")
    assert {k: cg[k] for k in RAY_KEYS} == {k: cref[k] for k in RAY_KEYS}, label
    _assert_bits(g[f.K], f.emission(lights), f"{label}: emission plane")
    for k in range(f.K):
        _assert_bits(g[k][..., :3], f.stripped(lights, k)[..., :3], f"{label}: light plane {k} RGB")
    for k in range(f.K + 1):
        _assert_bits(g[k][..., 3], out[..., 3], f"{label}: plane {k} w")
    # the test is not empty: every light lands somewhere, and the planes differ from each other
    for k in range(f.K):
        assert float(g[k][..., :3].sum()) > 0, (label, k)
    return out, g, f


@pytest.fixture(scope="module")
def atrium(pkg):
    scene = pkg.Scene.atrium(1, 262144)
    yield scene
    scene.close()


def _pipe(pkg, scene, W=256, H=144, D=8, mat=0, **kw):
    pipe = pkg.FramePipeline(scene, W, H, max_depth=D, mat_index=mat, **kw)
    pipe.ctx.set_environment(color=(0.3, 0.45, 0.7, 1.0))  # (what ENV_ON_MISS finds)
    return pipe


def test_out_emission_and_light_planes_atrium_depth8(pkg, atrium):
    """(1)-(3) on the atrium (three lights, emissive lamp bodies) at 256x144, depth 8, GGX, two frames; and (2) with
    ENV_ON_MISS | EMISSIVE_HITS, whose terms belong to the emission plane only."""
    pipe = _pipe(pkg, atrium)
    for frame in range(2):
        _check_contract(pkg, pipe, 0, f"atrium frame {frame}")
        pipe.gbuffer_frame += 1
        pipe.bdpt_frame += 1
    out, g, f = _check_contract(pkg, pipe, EXT, "atrium EXT")
    plain, _ = f.plain(f.p)
    no_ext = pkg.abi.Params()
    C.pointer(no_ext)[0] = f.p
    no_ext.flags = 0
    assert not np.array_equal(_bits(plain), _bits(f.plain(no_ext)[0]))  # the extra terms are there
    pipe.close()


@pytest.mark.parametrize("variant", ["mis_power", "lambert", "depth16"])
def test_light_planes_variants(pkg, atrium, variant):
    """(4): (1)-(3) with BDPT_PARAM_MIS_POWER, with the Lambertian model, and at depth 16 (the 16-lane generators)."""
    if variant == "mis_power":
        pipe, flags = _pipe(pkg, atrium, W=160, H=96), 64
    elif variant == "lambert":
        pipe, flags = _pipe(pkg, atrium, W=160, H=96, mat=1), 0
    else:
        pipe, flags = _pipe(pkg, atrium, W=128, H=80, D=16), 0
    _check_contract(pkg, pipe, flags, variant)
    pipe.close()


def test_directional_and_spot_lights_against_oracle(pkg, ob):
    """(5): a scene edited by bdpt_set_lights to hold a directional light and a spot light; (1)-(3) on the GPU, and
    every light plane's RGB against the CPU oracle rendering the stripped scene on the stripped G-buffer."""
    import torch
    scene = pkg.Scene.atrium(2, 20000)
    lights = _copy_lights(pkg, scene.desc)
    assert len(lights) == 3
    lights[1].type = pkg.abi.LIGHT_DIRECTIONAL
    lights[1].dirW[0], lights[1].dirW[1], lights[1].dirW[2] = 0.3, -0.9, 0.3
    lights[1].intensity[0], lights[1].intensity[1], lights[1].intensity[2] = 1.5, 1.4, 1.2
    assert lights[2].openingAngle < 3.0  # the atrium's spot light
    pipe = _pipe(pkg, scene, W=64, H=64, D=5)
    pipe.set_lights(lights)
    out, g, f = _check_contract(pkg, pipe, 0, "directional + spot", lights)
    for k in range(f.K):
        only = _only(pkg, lights, k)
        arr = (pkg.abi.Light * len(only))(*only)
        d = pkg.abi.SceneDesc()
        C.pointer(d)[0] = scene.desc
        d.lights = C.cast(arr, C.POINTER(pkg.abi.Light))
        orc = ob.OracleRender(pkg.abi, d, pipe.W, pipe.H)
        orc.gbuffer(pipe.cam, f.gp)
        orc.chan["emissive"][:, :3] = 0
        orc.chan["materialDiffuse"][orc.chan["worldPosition"][:, 3] == 0, :3] = 0
        orc.bdpt(pipe.cam, f.p)
        orc.resolve()
        ref = orc.image()[..., :3]
        _assert_bits(g[k][..., :3], ref, f"oracle, light {k}")
        orc.close()
    torch.cuda.synchronize()
    pipe.close()
    scene.close()


def test_planes_sum_to_out_on_a_dim_frame(pkg, atrium):
    """(6): with every light a hundred times dimmer no write saturates, and the planes add up to `out` within 1e-5."""
    pipe = _pipe(pkg, atrium, W=160, H=96)
    lights = _copy_lights(pkg, atrium.desc)
    for l in lights:
        for c in range(3):
            l.intensity[c] *= 0.01
    pipe.set_lights(lights)
    f = Frame(pkg, pipe)
    out, g, _ = f.groups()
    o = out.cpu().numpy()[..., :3].astype(np.float64)
    s = g.cpu().numpy()[..., :3].astype(np.float64).sum(axis=0)
    # a clamp leaves its channel at exactly 1 (every term is >= 0): where all three stay below 1, nothing clamped
    # (the emissive lamp bodies the camera sees directly may exceed 1 and clamp at a connection write)
    ok = o.max(axis=-1) < 1.0
    assert ok.mean() > 0.95, ok.mean()
    err = np.abs(s - o)[ok]
    assert np.all(err <= 1e-5 * np.abs(o[ok])), float(np.max(err / np.maximum(np.abs(o[ok]), 1e-30)))
    assert float((g[: f.K, ..., :3] > 0).float().mean()) > 0.05
    pipe.close()


def test_pipeline_accumulates_planes_as_stripped_frames(pkg):
    """(7): FramePipeline(light_groups=True) over 12 accumulated frames: every accumulated plane equals the running mean
    of the frames it stands for (rendered by a second context), and a set_lights after frame 6 restarts both."""
    import torch
    scene = pkg.Scene.atrium(3, 20000)
    W, H, D = 96, 64, 5
    pipe = _pipe(pkg, scene, W=W, H=H, D=D, light_groups=True)
    ref = _pipe(pkg, scene, W=W, H=H, D=D)
    K = int(scene.desc.numLights)
    assert tuple(pipe.light_groups.shape) == (K + 1, H, W, 4)
    lights = _copy_lights(pkg, scene.desc)
    last = [torch.zeros(H, W, 4, dtype=torch.float32, device=ref.dev) for _ in range(K + 1)]
    n = 0
    for frame in range(12):
        if frame == 6:
            for l in lights:
                l.posW[0] += 0.5
            pipe.set_lights(lights)
            ref.set_lights(lights)
            n = 0
        f = Frame(pkg, ref)  # the G-buffer of this frame on the reference context (same counters as pipe's)
        planes = [f.stripped(lights, k) for k in range(K)] + [f.emission(lights)]
        for k in range(K + 1):
            ref.ctx.accumulate(C.c_void_p(last[k].data_ptr()), C.c_void_p(planes[k].data_ptr()), n, pipe.accum_limit, W * H,
                               ref._stream_ptr())
        ref.gbuffer_frame += 1
        ref.bdpt_frame += 1
        n += 1
        pipe.render_frame(accumulate=True)
        torch.cuda.synchronize()
        _assert_bits(pipe.light_groups_accum, pipe.light_groups, f"frame {frame}: groups = their mean after accumulating")
        for k in range(K):
            _assert_bits(pipe.light_groups_accum[k][..., :3], last[k][..., :3], f"frame {frame}: accumulated light {k}")
        _assert_bits(pipe.light_groups_accum[K], last[K], f"frame {frame}: accumulated emission")
    pipe.close()
    ref.close()
    scene.close()


def test_captured_group_frame_replays_bit_exact(pkg, atrium):
    """(8): bdpt_prepare(BDPT_PREPARE_LIGHT_GROUPS), then a captured (G-buffer, group frame) replays to the bits of a
    direct call."""
    import torch
    pipe = _pipe(pkg, atrium, W=160, H=90, light_groups=True)
    pipe.ctx.prepare(pkg.abi.PREPARE_LIGHT_GROUPS)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        pipe.render_frame()
    torch.cuda.synchronize()
    ref_out, ref_g = pipe.output.clone(), pipe.light_groups.clone()
    pipe.gbuffer_frame, pipe.bdpt_frame = 0xdeadbeef, 0x1337
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        pipe.render_frame()
        graph.capture_end()
    torch.cuda.synchronize()
    for _ in range(2):
        pipe.output.zero_()
        pipe.light_groups.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _assert_bits(pipe.output, ref_out, "replayed out")
        _assert_bits(pipe.light_groups, ref_g, "replayed planes")
    del graph
    pipe.close()


def test_error_cases_on_a_real_context(pkg):
    """(9): no scene or size BDPT_E_STATE; a band or striped context, the DEFER flags, NULL groups BDPT_E_INVALID;
    capture without the prepare BDPT_E_STATE (and nothing enqueued); prepare without a scene BDPT_E_STATE."""
    import torch
    lib = pkg.load_library()
    scene = pkg.Scene.atrium(2, 20000)
    W, H = 64, 48
    K = int(scene.desc.numLights)
    out = torch.zeros(H, W, 4, dtype=torch.float32, device="cuda")
    g = torch.zeros(K + 1, H, W, 4, dtype=torch.float32, device="cuda")
    ctx = pkg.Context(0)
    p = pkg.abi.Params()
    p.maxDepth, p.clampUpper, p.minT = 3, 0.9, 1e-4
    gb = pkg.abi.GBuffer()

    def call(params=p, groups=g):
        return lib.bdpt_execute_light_groups(ctx._h, C.byref(params), C.byref(gb), C.c_void_p(out.data_ptr()),
                                             None if groups is None else C.c_void_p(groups.data_ptr()), None)

    assert call() == -2  # no scene, no size
    assert lib.bdpt_prepare(ctx._h, pkg.abi.PREPARE_LIGHT_GROUPS) == -2
    ctx.resize(W, H, 0, H, 3)
    assert lib.bdpt_prepare(ctx._h, pkg.abi.PREPARE_LIGHT_GROUPS) == -2  # (needs the scene: planes are per light)
    ctx.set_scene(scene.desc)
    ctx.set_camera(scene.camera(W / H))
    assert call(groups=None) == -1
    for fl in (pkg.abi.PARAM_DEFER_RESOLVE, pkg.abi.PARAM_DEFER_TAIL):
        q = pkg.abi.Params()
        C.pointer(q)[0] = p
        q.flags = fl
        assert call(q) == -1
    ctx.resize(W, H, 0, H // 2, 3)
    assert call() == -1 and "whole frame" in lib.bdpt_last_error(ctx._h).decode()
    ctx.resize_stripes(W, H, 4, 2, 0, 3)
    assert call() == -1
    ctx.resize_stripes(W, H, 4, 1, 0, 3)  # (stripes of one owner cover the frame, but they are still stripes)
    assert call() == -1
    # capture without the prepare: refused before anything is enqueued
    pipe = _pipe(pkg, scene, W=W, H=H, D=3, light_groups=True)
    side = torch.cuda.Stream()
    x = torch.zeros(16, device="cuda")
    with torch.cuda.stream(side):
        pipe.ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, pipe._stream_ptr())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        x.add_(1)
        with pytest.raises(pkg.BdptError, match="BDPT_PREPARE_LIGHT_GROUPS"):
            pipe.ctx.execute_light_groups(pipe.bdpt_params(), pipe.gb, C.c_void_p(pipe.output.data_ptr()),
                                          C.c_void_p(pipe.light_groups.data_ptr()), pipe._stream_ptr())
        graph.capture_end()
    torch.cuda.synchronize()
    del graph
    pipe.close()
    ctx.close()
    scene.close()
