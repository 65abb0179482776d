"""GPU tests of the context's lifetimes (csrc/context.hpp): what bdpt_set_scene, bdpt_resize, bdpt_set_skin and
bdpt_set_morph drop, as include/bdpt.h promises it, and that a context which carried every optional piece of state
renders, after the drop, what a fresh context renders: the G-buffer channels and the BDPT frame, bit for bit.  Cornell
box, 16 x 16 pixels, depth 2; every image is compared as float words viewed as integers."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library is loaded, as test_gpu_gi.py explains)

pytestmark = pytest.mark.gpu

W = H = 16
BIG = 24  # the other frame size (the same aspect: the camera stays)
DEPTH = 2
E_STATE = -2


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


class Rig:
    """A context with a w x h whole-frame tile, and one fixed G-buffer pass + BDPT frame on buffers of its own"""

    def __init__(self, pkg, scene=None, w=W, h=H):
        self.pkg, self.abi, self.ctx = pkg, pkg.abi, pkg.Context(0)
        self.resize(w, h)
        if scene is not None:
            self.set_scene(scene)

    def resize(self, w, h):
        self.ctx.resize(w, h, 0, h, DEPTH)
        self.w, self.h = w, h

    def set_scene(self, scene, desc=None):
        self.ctx.set_scene(scene.desc if desc is None else desc)
        self.ctx.set_camera(scene.camera(1.0))

    def _buffers(self):
        chans = [torch.zeros(self.h, self.w, 4, dtype=torch.float32, device="cuda")]
        chans += [torch.zeros(self.h, self.w, 4, dtype=torch.float16, device="cuda") for _ in range(5)]
        return chans, self.abi.GBuffer(*[c.data_ptr() for c in chans]), torch.zeros(self.h, self.w, 4, dtype=torch.float32, device="cuda")

    def params(self, flags=0):
        gp = self.abi.GBufferParams()
        gp.pixelJitter[0] = gp.pixelJitter[1] = 0.5
        gp.frameCount, gp.focalLen, gp.lensRadius = 7, 1.0, 1.0 / 64.0
        gp.envWidth = gp.envHeight = 128
        gp.envColor[0], gp.envColor[1], gp.envColor[2], gp.envColor[3] = 0.5, 0.5, 0.8, 1.0
        p = self.abi.Params()
        p.minT, p.frameCount, p.matIndex, p.refractiveIndex, p.maxDepth, p.emitMult, p.clampUpper = 1e-4, 0x1337, 0, 1.0, DEPTH, 1.0, 0.9
        p.pixelJitter[0] = p.pixelJitter[1] = 0.5
        p.flags = flags
        return gp, p

    def frame(self):
        """[six G-buffer channels, the BDPT frame over them, the BDPT frame over the built-in primary stage] as numpy"""
        chans, gb, out = self._buffers()
        own = torch.zeros_like(out)
        gp, p = self.params()
        self.ctx.gbuffer_execute(gp, gb, _stream())
        self.ctx.execute(p, gb, _ptr(out), _stream())
        self.ctx._check(self.ctx._lib.bdpt_execute(self.ctx._h, C.byref(p), None, _ptr(own), _stream()), "bdpt_execute(in = NULL)")
        torch.cuda.synchronize()
        return [c.cpu().numpy() for c in chans] + [out.cpu().numpy(), own.cpu().numpy()]

    def code(self, fn, *args, **kw):
        """the error code a refused binding call carries in its BdptError, or 0"""
        try:
            fn(*args, **kw)
        except self.pkg.BdptError as e:
            return int(str(e).split("(")[1].split(")")[0])
        return 0

    def history_bytes(self):
        n = C.c_uint64(123)
        assert self.ctx._lib.bdpt_bmfr_history_bytes(self.ctx._h, C.byref(n)) == 0
        return n.value

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def scenes(pkg):
    a, b = pkg.Scene.cornell(), pkg.Scene.soup(5, 300)
    assert b.desc.numLights >= 1 and b.desc.numVertices != a.desc.numVertices
    yield a, b
    a.close()
    b.close()


@pytest.fixture(scope="module")
def fresh(pkg, scenes):
    """what a fresh context renders: scene A at both sizes, scene B at the small one (computed once, read only)"""
    a, b = scenes
    want = {}
    for name, scene, size in (("a", a, W), ("a_big", a, BIG), ("b", b, W)):
        rig = Rig(pkg, scene, size, size)
        want[name] = rig.frame()
        rig.close()
    assert not _same(want["a"], want["b"]) and np.isfinite(want["a"][6]).all() and want["a"][6][..., :3].max() > 0.0
    return want


def _skin_and_morph(rig, scene):
    """a one-bone skin over the scene's own vertices (identity palette: the pose stays) and a one-entry morph"""
    nv = int(scene.desc.numVertices)
    pos = np.ctypeslib.as_array(scene.desc.positions, (nv * 3,)).copy()
    w = np.zeros((nv, 4), np.float32)
    w[:, 0] = 1.0
    rig.ctx.set_skin(pos, w, np.zeros((nv, 4), np.uint16), 1)
    rig.ctx.set_morph(np.array([0, 1], np.uint32), np.array([0], np.uint32), np.zeros((1, 3), np.float32))


def _load(rig, scene, update):
    """every optional piece of scene and frame state: skin, morph, refit plan (and one update, with the identity: only
    where the scene is replaced afterwards, since a refitted tree is not the built one), previous pose, emitter table,
    light-group planes, the own G-buffer, a BMFR history with one denoised frame in it"""
    abi = rig.abi
    _skin_and_morph(rig, scene)
    rig.ctx.prepare(abi.PREPARE_REFIT | abi.PREPARE_AREA_LIGHTS | abi.PREPARE_LIGHT_GROUPS | abi.PREPARE_PRIMARY | abi.PREPARE_BMFR, motion=True)
    if update:
        rig.ctx.update_morphed(np.zeros(1, np.float32), np.eye(4, dtype=np.float32).reshape(1, 16))
        assert rig.ctx.refit_info().numUpdates == 1
    chans, gb, out = rig._buffers()
    gp, p = rig.params()
    rig.ctx.gbuffer_execute(gp, gb, _stream())
    nl = int(scene.desc.numLights)
    groups = torch.zeros(nl + 1, rig.h, rig.w, 4, dtype=torch.float32, device="cuda")
    rig.ctx.execute_light_groups(p, gb, _ptr(out), _ptr(groups), _stream())
    bp = abi.BmfrParams()
    bp.frameNumber, bp.flags = 0, abi.BMFR_PREPROCESS | abi.BMFR_REGRESSION | abi.BMFR_POSTPROCESS
    for i in range(16):
        bp.prevViewProj[i] = float(i % 5 == 0)
    rig.ctx.bmfr_execute(bp, gb, _ptr(out), _stream())
    torch.cuda.synchronize()
    assert rig.history_bytes() == rig.w * rig.h * 16 * 4
    assert all(rig.ctx.skinned_buffers()[:1]) and rig.ctx.morphed_buffers()[0]


def _refused_after_scene_drop(rig):
    hits = torch.zeros(4, 4, dtype=torch.float32, device="cuda")
    assert rig.code(rig.ctx.skinned_buffers) == E_STATE
    assert rig.code(rig.ctx.morphed_buffers) == E_STATE
    assert rig.code(rig.ctx.motion_query, hits) == E_STATE
    assert rig.code(rig.ctx.update_skinned, np.eye(4, dtype=np.float32).reshape(1, 16)) == E_STATE
    assert rig.code(rig.ctx.update_morphed, np.zeros(1, np.float32)) == E_STATE
    assert rig.ctx.refit_info().numUpdates == 0


def _set_scene_sequence(pkg, scenes, fresh):
    a, b = scenes
    rig = Rig(pkg, a)
    _load(rig, a, update=True)
    rig.set_scene(b)
    _refused_after_scene_drop(rig)
    assert _same(rig.frame(), fresh["b"])
    return rig


def _resize_sequence(pkg, scenes, fresh):
    a, _ = scenes
    rig = Rig(pkg, a)
    _load(rig, a, update=False)
    first = rig.frame()
    assert _same(first, fresh["a"])
    rig.resize(BIG, BIG)
    assert rig.history_bytes() == 0
    assert _same(rig.frame(), fresh["a_big"])
    rig.resize(W, H)
    assert rig.history_bytes() == 0
    assert _same(rig.frame(), first)
    return rig


def test_set_scene_drops_what_hangs_on_the_scene(pkg, scenes, fresh):
    _set_scene_sequence(pkg, scenes, fresh).close()


def test_resize_drops_what_hangs_on_the_frame(pkg, scenes, fresh):
    _resize_sequence(pkg, scenes, fresh).close()


def test_skin_drops_the_morph_and_the_morph_leaves_the_skin(pkg, scenes):
    a, _ = scenes
    rig = Rig(pkg, a)
    _skin_and_morph(rig, a)
    rig.ctx.set_skin(None, None, None, 0)
    assert rig.code(rig.ctx.morphed_buffers) == E_STATE and rig.code(rig.ctx.skinned_buffers) == E_STATE
    _skin_and_morph(rig, a)
    rig.ctx.set_morph(None, None, None)
    assert rig.code(rig.ctx.morphed_buffers) == E_STATE
    assert rig.ctx.skinned_buffers()[0]
    rig.close()


def test_a_failing_set_scene(pkg, scenes, fresh):
    """refused by validation: the old scene stays; refused after the drop point: the context has no scene"""
    a, b = scenes
    abi = pkg.abi
    rig = Rig(pkg, a)
    assert _same(rig.frame(), fresh["a"])
    bad = abi.SceneDesc.from_buffer_copy(b.desc)
    tri_mat = np.full(int(b.desc.numTriangles), int(b.desc.numMaterials), np.uint32)
    bad.triMaterial = tri_mat.ctypes.data_as(C.POINTER(C.c_uint32))
    with pytest.raises(pkg.BdptError, match="triMaterial out of range"):
        rig.ctx.set_scene(bad)
    assert _same(rig.frame(), fresh["a"])
    bad = abi.SceneDesc.from_buffer_copy(b.desc)
    tex = (abi.Texture * max(1, int(b.desc.numTextures)))()  # (every material's texture index stays in range)
    pixel = (C.c_uint8 * 4)()
    for t in tex:
        t.rgba8, t.width, t.height = pixel, 0, 1
    bad.numTextures, bad.textures = len(tex), tex
    with pytest.raises(pkg.BdptError, match="empty texture"):
        rig.ctx.set_scene(bad)
    rays = torch.zeros(1, 8, dtype=torch.float32, device="cuda")
    assert rig.code(rig.ctx.trace_rays, rays) == E_STATE
    rig.set_scene(b)
    assert _same(rig.frame(), fresh["b"])
    rig.close()


def test_two_contexts_through_every_sequence(pkg, scenes, fresh):
    rigs = [_set_scene_sequence(pkg, scenes, fresh), _resize_sequence(pkg, scenes, fresh)]
    rigs += [_resize_sequence(pkg, scenes, fresh), _set_scene_sequence(pkg, scenes, fresh)]
    for rig in rigs:
        rig.close()
    torch.cuda.synchronize()
    assert torch.zeros(1, device="cuda").item() == 0.0  # (the runtime is still in order)
