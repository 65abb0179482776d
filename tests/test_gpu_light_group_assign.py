"""GPU tests of bdpt_execute_grouped (contract: include/bdpt.h "Assignable light groups").  Every comparison is on raw
bits: `out` and the ray counters against bdpt_execute's, a group plane's RGB against the bdpt_execute frame in which every
source outside the group contributes +0 (point lights: intensity zero; the emitter table: a second scene whose emission
textures are black, which leaves the table, the draws and the rays as they are), on the stripped G-buffer (emissive RGB
zero, background diffuse RGB zero) with ENV_ON_MISS / EMISSIVE_HITS cleared, the method of tests/test_gpu_light_groups.py.
Every test also asserts that it is not empty: the non-empty group planes have a positive RGB sum and differ from each
other."""
import ctypes as C

import numpy as np
import pytest

from area_scenes import (AREA, DEFER_RESOLVE, DEFER_TAIL, EMISSIVE_HITS, ENV_ON_MISS, MIS_POWER, NO_CONNECT, NO_NEE, NO_SPLAT,
                         AreaScene, DescArrays)

pytestmark = pytest.mark.gpu

RAY_KEYS = ("raysPrimary", "raysEyeExtend", "raysLightExtend", "raysNee", "raysSplat", "raysConnect", "pixelsValid",
            "splatsLanded", "raysConnectLazy", "hintedNee", "hintedSplat")
EXT = ENV_ON_MISS | EMISSIVE_HITS
MIS_LINEAR = 128
GB_NAMES = ["WorldPosition", "WorldNormal", "MaterialDiffuse", "MaterialSpecRough", "MaterialExtraParams", "Emissive"]
SENTINEL = 7.0  # (a value no frame writes)


def _bits(t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_bits(a, b, label):
    x, y = _bits(a), _bits(b)
    assert x.shape == y.shape, label
    if not np.array_equal(x, y):
        bad = (x != y).reshape(-1, x.shape[-1]).any(axis=-1).sum()
        raise AssertionError(f"{label}: {bad} pixels differ")


def _rays(c):
    return {k: c[k] for k in RAY_KEYS}


def _copy_lights(pkg, desc):
    out = [pkg.abi.Light() for _ in range(desc.numLights)]
    for i in range(desc.numLights):
        C.memmove(C.byref(out[i]), C.byref(desc.lights[i]), C.sizeof(pkg.abi.Light))
    return out


def _lit(pkg, lights, keep):
    """The lights with every intensity zero but those of the indices in `keep`."""
    out = []
    for i, l in enumerate(lights):
        m = pkg.abi.Light()
        C.memmove(C.byref(m), C.byref(l), C.sizeof(pkg.abi.Light))
        if i not in keep:
            m.intensity[0] = m.intensity[1] = m.intensity[2] = 0.0
        out.append(m)
    return out


def _params(pkg, p, flags):
    q = pkg.abi.Params()
    C.pointer(q)[0] = p
    q.flags = flags
    return q


class Frame:
    """One pipeline's G-buffer of one frame and the renders the tests compare, all with the same params."""

    def __init__(self, pkg, pipe, flags=0):
        import torch
        self.pkg, self.pipe, self.torch = pkg, pipe, torch
        self.gp = pipe.gbuffer_params()
        pipe.ctx.gbuffer_execute(self.gp, pipe.gb, pipe._stream_ptr())
        self.p = pipe.bdpt_params(flags)
        self.K = int(pipe.scene.desc.numLights)
        self.lights = _copy_lights(pkg, pipe.scene.desc)
        ch = pipe.channels
        self.em0 = ch["Emissive"].clone()
        self.em0[..., :3] = 0
        self.dif0 = ch["MaterialDiffuse"].clone()
        self.dif0[..., :3][ch["WorldPosition"][..., 3] == 0] = 0
        t = {n: ch[n] for n in GB_NAMES}
        t["MaterialDiffuse"], t["Emissive"] = self.dif0, self.em0
        self.gb0 = pkg.abi.GBuffer(*[t[n].data_ptr() for n in GB_NAMES])  # the stripped G-buffer
        torch.cuda.synchronize()

    def _new(self, planes=None):
        shape = (self.pipe.H, self.pipe.W, 4) if planes is None else (planes, self.pipe.H, self.pipe.W, 4)
        return self.torch.full(shape, SENTINEL, dtype=self.torch.float32, device=self.pipe.dev)

    def plain(self, params=None, gb=None, pipe=None):
        pipe = pipe or self.pipe
        out = self._new()
        pipe.ctx.execute(params or self.p, gb or self.pipe.gb, C.c_void_p(out.data_ptr()), pipe._stream_ptr())
        self.torch.cuda.synchronize()
        return out, pipe.ctx.counters().as_dict()

    def grouped(self, assignment, num_groups=None, params=None):
        n = max(assignment) + 1 if num_groups is None else num_groups
        out, g = self._new(), self._new(n + 1)
        self.pipe.ctx.execute_grouped(params or self.p, self.pipe.gb, C.c_void_p(out.data_ptr()), C.c_void_p(g.data_ptr()),
                                      assignment, n, self.pipe._stream_ptr())
        self.torch.cuda.synchronize()
        return out, g, self.pipe.ctx.counters().as_dict()

    def old_groups(self):
        out, g = self._new(), self._new(self.K + 1)
        self.pipe.ctx.execute_light_groups(self.p, self.pipe.gb, C.c_void_p(out.data_ptr()), C.c_void_p(g.data_ptr()),
                                           self.pipe._stream_ptr())
        self.torch.cuda.synchronize()
        return out, g, self.pipe.ctx.counters().as_dict()

    def only(self, keep, pipe=None, stripped=True, gb=None):
        """bdpt_execute with only the point lights `keep` lit; stripped: on the stripped G-buffer, without EXT."""
        pipe = pipe or self.pipe
        st = pipe._stream_ptr()
        pipe.ctx.set_lights(_lit(self.pkg, self.lights, keep), st)
        p = _params(self.pkg, self.p, self.p.flags & ~EXT) if stripped else self.p
        out, _ = self.plain(p, gb or (self.gb0 if stripped else self.pipe.gb), pipe)
        pipe.ctx.set_lights(self.lights, st)
        return out


def _assert_not_empty(g, n, label, empty=()):
    full = [k for k in range(n) if k not in empty]
    for k in full:
        assert float(g[k][..., :3].sum()) > 0, (label, "group plane is black", k)
    for k in empty:
        assert float(g[k][..., :3].abs().sum()) == 0, (label, "empty group has light", k)
    for i in range(len(full)):
        for j in range(i + 1, len(full)):
            assert not np.array_equal(_bits(g[full[i]][..., :3]), _bits(g[full[j]][..., :3])), (label, "planes equal", full[i], full[j])


def _assert_w(g, out, label):
    for k in range(g.shape[0]):
        _assert_bits(g[k][..., 3], out[..., 3], f"{label}: plane {k} w")


@pytest.fixture(scope="module")
def atrium(pkg):
    scene = pkg.Scene.atrium(1, 262144)
    yield scene
    scene.close()


@pytest.fixture(scope="module")
def cornell(pkg):
    s = pkg.Scene.cornell()
    yield s
    s.close()


def _pipe(pkg, scene, W=256, H=144, D=8, mat=0, **kw):
    pipe = pkg.FramePipeline(scene, W, H, max_depth=D, mat_index=mat, **kw)
    pipe.ctx.set_environment(color=(0.3, 0.45, 0.7, 1.0))  # (what ENV_ON_MISS finds)
    return pipe


# ---- (1) the identity assignment is the old call
@pytest.mark.parametrize("flags", [0, EXT])
def test_identity_equals_execute_light_groups(pkg, atrium, flags):
    pipe = _pipe(pkg, atrium)
    f = Frame(pkg, pipe, flags)
    assert f.K == 3
    out0, g0, c0 = f.old_groups()
    out1, g1, c1 = f.grouped([0, 1, 2])
    _assert_bits(out1, out0, "out")
    _assert_bits(g1, g0, "planes")
    assert _rays(c1) == _rays(c0)
    _assert_not_empty(g1, 3, "identity")
    pipe.close()


# ---- (2) merged groups
def _check_merged(pkg, pipe, flags, assignment, label, num_groups=None):
    f = Frame(pkg, pipe, flags)
    ref, cref = f.plain()
    out, g, cg = f.grouped(assignment, num_groups)
    n = g.shape[0] - 1
    _assert_bits(out, ref, f"{label}: out")
    assert _rays(cg) == _rays(cref), label
    for k in range(n):
        keep = [i for i, a in enumerate(assignment) if a == k]
        _assert_bits(g[k][..., :3], f.only(keep)[..., :3], f"{label}: group {k} RGB")
    _assert_bits(g[n], f.only([], stripped=False), f"{label}: emission plane")
    _assert_w(g, out, label)
    return g, n


@pytest.mark.parametrize("flags", [0, EXT])
def test_merged_groups_atrium_depth8(pkg, atrium, flags):
    pipe = _pipe(pkg, atrium)
    g, n = _check_merged(pkg, pipe, flags, [0, 1, 0], "[0, 1, 0]")
    _assert_not_empty(g, n, "[0, 1, 0]")
    g1, n1 = _check_merged(pkg, pipe, flags, [0, 0, 0], "[0, 0, 0]")
    _assert_not_empty(g1, n1, "[0, 0, 0]")
    assert not np.array_equal(_bits(g1[0][..., :3]), _bits(g[0][..., :3]))  # (light 1 is in the one and not in the other)
    # an empty group in the middle: its plane is (0, 0, 0, w)
    g2, n2 = _check_merged(pkg, pipe, flags, [2, 0, 2], "[2, 0, 2]")
    _assert_not_empty(g2, n2, "[2, 0, 2]", empty=(1,))
    _assert_bits(g2[2], g[0], "group {0, 2} under another index")
    pipe.close()


@pytest.mark.parametrize("flags", [0, NO_NEE, NO_SPLAT, NO_CONNECT])
def test_merged_groups_small_lambertian(pkg, atrium, flags):
    pipe = _pipe(pkg, atrium, W=96, H=64, D=3, mat=1)
    for assignment in ([0, 1, 0], [0, 0, 0]):
        g, n = _check_merged(pkg, pipe, flags, assignment, f"{assignment} flags {flags}")
        _assert_not_empty(g, n, f"{assignment} flags {flags}")
    pipe.close()


# ---- (3) the emitter table as a source
def _textured_pair(pkg, cornell):
    """The relit Cornell box with every emitter of BDPT_CHANNEL_TEXTURE type (the ceiling patch, the floating textured
    quad and the alpha-masked quad), and the same description with the emission textures' RGB zero."""
    a = pkg.abi
    s = AreaScene(pkg, cornell, extra=True, point_light=True, relit=True)
    mats = []
    for i in range(len(s.mats)):
        m = a.Material()
        C.memmove(C.byref(m), C.byref(s.mats[i]), C.sizeof(a.Material))
        mats.append(m)
    textures = list(s.textures)
    emitters = [i for i, m in enumerate(mats) if ((m.flags >> 9) & 7) != 0]
    assert len(emitters) == 3
    texels = {3: (255, 240, 200, 255)}
    for i in emitters:
        m = mats[i]
        if ((m.flags >> 9) & 7) == 2:
            continue  # (the floating textured emitter, texture 0)
        t = np.zeros((2, 2, 4), np.uint8)
        t[...] = texels.get(i, (230, 120, 60, 255))
        textures.append((t, True))
        m.texEmissive = len(textures) - 1
        m.flags = (m.flags & ~(7 << 9)) | (2 << 9)
    assert any(((m.flags >> 17) & 3) != 0 for m in (mats[i] for i in emitters))  # one of them alpha-masked
    em_tex = sorted({mats[i].texEmissive for i in emitters})
    black = []
    for k, (t, srgb) in enumerate(textures):
        t = t.copy()
        if k in em_tex:
            t[..., :3] = 0
        black.append((t, srgb))
    lights = list(s.lights)
    sa = DescArrays(a, s.P, s.N, s.T, s.I, s.M, mats, textures, lights)
    sb = DescArrays(a, s.P, s.N, s.T, s.I, s.M, mats, black, lights)
    for x in (sa, sb):
        x.camera = s.base.camera
        x.keep = s
    return sa, sb


@pytest.mark.parametrize("depth, mat", [(3, 0), (3, 1), (8, 0), (8, 1)])
def test_table_as_a_source(pkg, cornell, depth, mat):
    sa, sb = _textured_pair(pkg, cornell)
    pa = _pipe(pkg, sa, W=96, H=64, D=depth, mat=mat)
    pb = _pipe(pkg, sb, W=96, H=64, D=depth, mat=mat)
    ia, ib = pa.ctx.area_light_info(), pb.ctx.area_light_info()
    assert ia.numEmitters == ib.numEmitters == ia.numTextured > 0 and ia.totalWeight == ib.totalWeight > 0
    K = 4
    for flags in (AREA, AREA | EMISSIVE_HITS):
        f = Frame(pkg, pa, flags)
        assert f.K == K
        ref, cref = f.plain()
        assert not np.array_equal(_bits(ref), _bits(f.plain(_params(pkg, f.p, flags & ~AREA))[0]))  # the switch is live
        table_only = f.only([])           # scene A, every point light dark: the table alone
        light_only = [f.only([k], pipe=pb) for k in range(K)]  # scene B (black table), one point light each
        for assignment in ([0, 1, 2, 3, 4], [0, 1, 2, 3, 0]):
            label = f"depth {depth} mat {mat} flags {flags} {assignment}"
            out, g, cg = f.grouped(assignment)
            n = g.shape[0] - 1
            _assert_bits(out, ref, f"{label}: out")
            assert _rays(cg) == _rays(cref), label
            _assert_w(g, out, label)
            if n == 5:
                _assert_bits(g[4][..., :3], table_only[..., :3], f"{label}: the table's plane")
                _assert_bits(g[0][..., :3], light_only[0][..., :3], f"{label}: light 0")
            else:
                _assert_bits(g[0][..., :3], f.only([0])[..., :3], f"{label}: light 0 with the table")
                assert not np.array_equal(_bits(g[0][..., :3]), _bits(light_only[0][..., :3]))
            for k in range(1, K):
                _assert_bits(g[k][..., :3], light_only[k][..., :3], f"{label}: light {k}")
            if not (flags & EMISSIVE_HITS):
                # every source at +0: scene B, every point light dark, on scene A's own G-buffer
                _assert_bits(g[n], f.only([], pipe=pb, stripped=False), f"{label}: emission plane")
            # (with EMISSIVE_HITS and a live table no bdpt_execute frame equals the emission plane: the walk's term and
            # the table read one emission, so a scene cannot keep the first and darken the second.  `out`, the group
            # planes and w are asserted above.)
            _assert_not_empty(g, n, label)
    pa.close()
    pb.close()


# ---- (4), (6) constant, masked and dropped emitters; the same after bdpt_update_geometry
def _check_const_table(pkg, pipe, label):
    f = Frame(pkg, pipe, AREA)
    assert f.K == 1
    ref, cref = f.plain()
    assert not np.array_equal(_bits(ref), _bits(f.plain(_params(pkg, f.p, 0))[0]))  # the switch is live
    out, g, cg = f.grouped([0, 1])
    _assert_bits(out, ref, f"{label}: out")
    assert _rays(cg) == _rays(cref), label
    _assert_bits(g[1][..., :3], f.only([])[..., :3], f"{label}: the table's plane")
    _assert_w(g, out, label)
    _assert_not_empty(g, 2, label)
    out1, g1, c1 = f.grouped([0, 0])
    _assert_bits(out1, ref, f"{label}: out, one group")
    _assert_bits(g1[0][..., :3], f.only([0])[..., :3], f"{label}: light and table in one group")
    _assert_w(g1, out1, label)
    return ref


def test_constant_masked_and_dropped_emitters(pkg, cornell):
    scene = AreaScene(pkg, cornell, const_extra=True, transparent=True, point_light=True)
    pipe = _pipe(pkg, scene, W=96, H=64, D=5)
    assert pipe.ctx.bvh_info().numDropped == len(scene.dropped) > 0
    _check_const_table(pkg, pipe, "const")
    pipe.close()


def test_after_update_geometry(pkg, cornell):
    import torch
    scene = AreaScene(pkg, cornell, const_extra=True, transparent=True, point_light=True)
    pipe = _pipe(pkg, scene, W=96, H=64, D=5)
    before = _check_const_table(pkg, pipe, "before the update")
    w0 = pipe.ctx.area_light_info().totalWeight
    P = scene.P.copy()
    patch = np.unique(scene.I[scene.M == 3])
    c = P[patch].mean(axis=0)
    P[patch] = (P[patch] - c) * np.array([1.5, 1.0, 1.5], np.float32) + c + np.array([30.0, -20.0, 10.0], np.float32)
    pipe.update_geometry(torch.from_numpy(np.ascontiguousarray(P)).cuda())
    torch.cuda.synchronize()
    assert pipe.ctx.area_light_info().totalWeight > w0  # the table's weights were refreshed
    after = _check_const_table(pkg, pipe, "after the update")
    assert not np.array_equal(_bits(before), _bits(after))
    pipe.close()


# ---- (5) no table: the switch changes nothing and entry numLights is ignored
@pytest.mark.parametrize("kind", ["no_emitters", "zero_area"])
def test_no_table(pkg, cornell, kind):
    if kind == "no_emitters":
        scene = AreaScene(pkg, cornell, patch_emission=(0.0, 0.0, 0.0), extra=False, point_light=True)
    else:
        probe = AreaScene(pkg, cornell, extra=False, point_light=True)
        P = probe.P.copy()
        patch = np.unique(probe.I[probe.M == 3])
        P[patch] = P[patch[0]]  # the patch collapsed to a point: its emitters have zero area, exactly
        scene = AreaScene(pkg, cornell, extra=False, point_light=True, positions=P[: cornell.desc.numVertices])
        assert np.all(scene.P[patch] == scene.P[patch[0]])
    pipe = _pipe(pkg, scene, W=96, H=64, D=5)
    info = pipe.ctx.area_light_info()
    if kind == "no_emitters":
        assert info.numEmitters == 0
    else:
        assert info.numEmitters > 0 and info.totalWeight == 0.0
    f = Frame(pkg, pipe, 0)
    out0, g0, c0 = f.grouped([0], num_groups=2)
    out1, g1, c1 = f.grouped([0, 1], num_groups=2, params=_params(pkg, f.p, AREA))
    _assert_bits(out1, out0, kind)
    _assert_bits(g1, g0, kind)
    assert _rays(c1) == _rays(c0)
    _assert_bits(out0, f.plain()[0], kind)
    _assert_not_empty(g0, 2, kind, empty=(1,))
    pipe.close()


# ---- (7) capture
def test_captured_grouped_frame_replays_bit_exact(pkg, cornell):
    import torch
    scene = AreaScene(pkg, cornell, const_extra=True, point_light=True, relit=True)
    assignment = [0, 1, 0, 1, 2]
    pipe = _pipe(pkg, scene, W=96, H=64, D=5, flags=AREA, light_groups=assignment)
    assert tuple(pipe.light_groups.shape) == (4, 64, 96, 4)
    a = pkg.abi
    pipe.ctx.prepare(a.PREPARE_LIGHT_GROUP_TABLE | a.PREPARE_AREA_LIGHTS | a.PREPARE_PRIMARY)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        pipe.render_frame()
    torch.cuda.synchronize()
    ref_out, ref_g = pipe.output.clone(), pipe.light_groups.clone()
    _assert_not_empty(ref_g, 3, "captured")
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


def test_capture_without_the_prepare_is_refused(pkg, cornell):
    import torch
    scene = AreaScene(pkg, cornell, const_extra=True, point_light=True, relit=True)
    pipe = _pipe(pkg, scene, W=96, H=64, D=5, flags=AREA, light_groups=[0, 1, 0, 1, 2])
    pipe.ctx.prepare(pkg.abi.PREPARE_AREA_LIGHTS | pkg.abi.PREPARE_PRIMARY)
    side = torch.cuda.Stream()
    x = torch.zeros(16, device="cuda")
    with torch.cuda.stream(side):
        pipe.ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, pipe._stream_ptr())
    torch.cuda.synchronize()
    pipe.output.fill_(SENTINEL)
    pipe.light_groups.fill_(SENTINEL)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        x.add_(1)
        with pytest.raises(pkg.BdptError, match="BDPT_E_STATE|stream capture"):
            pipe.ctx.execute_grouped(pipe.bdpt_params(), pipe.gb, C.c_void_p(pipe.output.data_ptr()),
                                     C.c_void_p(pipe.light_groups.data_ptr()), pipe.group_assignment, 3, pipe._stream_ptr())
        graph.capture_end()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert float(x.sum()) == 16.0  # the graph holds the add (run once, by the replay) and nothing of the refused call
    assert bool((pipe.output == SENTINEL).all()) and bool((pipe.light_groups == SENTINEL).all())
    del graph
    pipe.close()


# ---- (8) errors, on a real context; nothing is enqueued
def test_error_cases_on_a_real_context(pkg, cornell):
    import torch
    lib = pkg.load_library()
    a = pkg.abi
    scene = AreaScene(pkg, cornell, point_light=True, relit=True)
    W, H, K = 64, 48, 4
    out = torch.full((H, W, 4), SENTINEL, dtype=torch.float32, device="cuda")
    g = torch.full((K + 2, H, W, 4), SENTINEL, dtype=torch.float32, device="cuda")
    ctx = pkg.Context(0)
    p = a.Params()
    p.maxDepth, p.clampUpper, p.minT = 3, 0.9, 1e-4
    chans = [torch.zeros(H, W, 4, dtype=torch.float32 if n == "WorldPosition" else torch.float16, device="cuda") for n in GB_NAMES]
    gb = a.GBuffer(*[t.data_ptr() for t in chans])

    def call(assignment=(0, 1, 2, 3), num_groups=4, flags=0, planes=True, group_of=True, desc=True, reserved=(0, 0), num_assigned=None,
             handle=True):
        arr = (C.c_uint8 * max(len(assignment), 1))(*assignment)
        d = a.LightGroupDesc()
        d.planes = g.data_ptr() if planes else None
        d.numGroups = num_groups
        d.numAssigned = len(assignment) if num_assigned is None else num_assigned
        d.groupOf = C.cast(arr, C.POINTER(C.c_uint8)) if group_of else None
        d.reserved[0], d.reserved[1] = reserved
        q = _params(pkg, p, flags)
        return lib.bdpt_execute_grouped(ctx._h if handle else None, C.byref(q), C.byref(gb), C.c_void_p(out.data_ptr()),
                                        C.byref(d) if desc else None, None)

    assert call() == -2  # no scene, no size
    assert lib.bdpt_prepare(ctx._h, a.PREPARE_LIGHT_GROUP_TABLE) == -2
    ctx.resize(W, H, 0, H, 3)
    assert call() == -2  # no scene
    assert lib.bdpt_prepare(ctx._h, a.PREPARE_LIGHT_GROUP_TABLE) == -2  # (needs the scene: planes are per light)
    ctx.set_scene(scene.desc)
    ctx.set_camera(scene.camera(W / H))
    assert call(handle=False) == -1
    assert call(desc=False) == -1
    assert call(planes=False) == -1
    assert call(group_of=False) == -1
    assert call(num_groups=0) == -1
    assert call(num_groups=a.BDPT_MAX_LIGHTS + 2) == -1
    assert call(assignment=(0, 1, 2, 3, 0)) == -1            # numLights + 1 entries without the switch
    assert call(assignment=(0, 1, 2), num_groups=4) == -1
    assert call(flags=AREA) == -1                            # numLights entries with the switch
    assert call(assignment=(0, 1, 2, 3, 0, 0), flags=AREA) == -1
    assert call(assignment=(0, 1, 2, 4)) == -1 and "numGroups" in lib.bdpt_last_error(ctx._h).decode()
    assert call(assignment=(0, 1, 2, 3, 4), flags=AREA) == -1  # the table's entry is checked too
    assert call(reserved=(1, 0)) == -1
    assert call(reserved=(0, 1)) == -1
    for fl in (DEFER_RESOLVE, DEFER_TAIL):
        assert call(flags=fl) == -1
    for fl in (MIS_POWER, MIS_LINEAR):
        assert call(assignment=(0, 1, 2, 3, 0), flags=AREA | fl) == -1 and "AREA_LIGHTS" in lib.bdpt_last_error(ctx._h).decode()
    # bdpt_execute_light_groups keeps refusing the switch, with its message
    q = _params(pkg, p, AREA)
    rc = lib.bdpt_execute_light_groups(ctx._h, C.byref(q), C.byref(gb), C.c_void_p(out.data_ptr()), C.c_void_p(g.data_ptr()), None)
    assert rc == -1 and "no slot for area lights" in lib.bdpt_last_error(ctx._h).decode()
    ctx.resize(W, H, 0, H // 2, 3)
    assert call() == -1 and "whole frame" in lib.bdpt_last_error(ctx._h).decode()
    ctx.resize_stripes(W, H, 4, 2, 0, 3)
    assert call() == -1
    ctx.resize_stripes(W, H, 4, 1, 0, 3)  # (stripes of one owner cover the frame, but they are still stripes)
    assert call() == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((g == SENTINEL).all())  # nothing was enqueued
    # and the same arguments, in order, do render (in == NULL: the context's own primary stage)
    ctx.resize(W, H, 0, H, 3)
    arr = (C.c_uint8 * 5)(0, 1, 2, 3, 4)
    d = a.LightGroupDesc()
    d.planes, d.numGroups, d.numAssigned, d.groupOf = g.data_ptr(), 5, 5, C.cast(arr, C.POINTER(C.c_uint8))
    q = _params(pkg, p, AREA)
    assert lib.bdpt_execute_grouped(ctx._h, C.byref(q), None, C.c_void_p(out.data_ptr()), C.byref(d), None) == 0
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any()) and not bool((g == SENTINEL).any())
    ctx.close()


# ---- (9) FramePipeline with a list, accumulated
def test_pipeline_accumulates_assigned_planes(pkg):
    """FramePipeline(light_groups=[0, 1, 0]) over 8 accumulated frames: every accumulated plane equals the running mean of
    the frames it stands for (rendered by a second context)."""
    import torch
    scene = pkg.Scene.atrium(3, 20000)
    W, H, D = 96, 64, 5
    assignment = [0, 1, 0]
    pipe = _pipe(pkg, scene, W=W, H=H, D=D, light_groups=assignment)
    ref = _pipe(pkg, scene, W=W, H=H, D=D)
    assert int(scene.desc.numLights) == 3
    assert tuple(pipe.light_groups.shape) == tuple(pipe.light_groups_accum.shape) == (3, H, W, 4)
    last = [torch.zeros(H, W, 4, dtype=torch.float32, device=ref.dev) for _ in range(3)]
    for frame in range(8):
        f = Frame(pkg, ref)  # the G-buffer of this frame on the reference context (same counters as pipe's)
        planes = [f.only([0, 2]), f.only([1]), f.only([], stripped=False)]
        for k in range(3):
            ref.ctx.accumulate(C.c_void_p(last[k].data_ptr()), C.c_void_p(planes[k].data_ptr()), frame, pipe.accum_limit, W * H,
                               ref._stream_ptr())
        ref.gbuffer_frame += 1
        ref.bdpt_frame += 1
        pipe.render_frame(accumulate=True)
        torch.cuda.synchronize()
        _assert_bits(pipe.light_groups_accum, pipe.light_groups, f"frame {frame}: groups = their mean after accumulating")
        for k in range(2):
            _assert_bits(pipe.light_groups_accum[k][..., :3], last[k][..., :3], f"frame {frame}: accumulated group {k}")
        _assert_bits(pipe.light_groups_accum[2], last[2], f"frame {frame}: accumulated emission")
    _assert_not_empty(pipe.light_groups_accum, 2, "accumulated")
    pipe.close()
    ref.close()
    scene.close()
