"""ctypes binding of oracle/liboracle.so — the CPU checker.  Test infrastructure only."""
import ctypes as C
import os

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_PATH = os.path.join(_ROOT, "oracle", "liboracle.so")
ORACLE_BRUTE_FORCE = 1
ORACLE_CONNECT_ALL_VISIBLE = 2
ORACLE_TERMS_ALL_VISIBLE = 4


class OracleFrame(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("y0", C.c_uint32), ("y1", C.c_uint32),
                ("worldPosition", C.c_void_p), ("worldNormal", C.c_void_p), ("materialDiffuse", C.c_void_p),
                ("materialSpecRough", C.c_void_p), ("materialExtra", C.c_void_p), ("emissive", C.c_void_p),
                ("out", C.c_void_p), ("splat", C.c_void_p)]


_lib = None


def load_oracle(abi):
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(ORACLE_PATH):
        raise RuntimeError(f"{ORACLE_PATH} missing: run `make -C oracle` (or __graft_entry__.build())")
    lib = C.CDLL(ORACLE_PATH)
    lib.oracle_scene_create.restype = C.c_void_p
    lib.oracle_scene_create.argtypes = [C.POINTER(abi.SceneDesc)]
    lib.oracle_scene_destroy.argtypes = [C.c_void_p]
    lib.oracle_set_environment.argtypes = [C.c_void_p, C.POINTER(abi.Environment)]
    lib.oracle_gbuffer.restype = C.c_int
    lib.oracle_gbuffer.argtypes = [C.c_void_p, C.POINTER(abi.Camera), C.POINTER(abi.GBufferParams), C.c_void_p,
                                   C.POINTER(OracleFrame), C.c_uint32, C.c_int]
    lib.oracle_bdpt.restype = C.c_int
    lib.oracle_bdpt.argtypes = [C.c_void_p, C.POINTER(abi.Camera), C.POINTER(abi.Params), C.POINTER(OracleFrame),
                                C.c_uint32, C.c_int, C.POINTER(abi.Counters)]
    lib.oracle_resolve.restype = C.c_int
    lib.oracle_resolve.argtypes = [C.POINTER(OracleFrame)]
    lib.oracle_accumulate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64]
    lib.oracle_rng.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.oracle_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.oracle_bsdf.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.oracle_shade_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.oracle_alpha_test.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.oracle_light_nee.argtypes = [C.POINTER(abi.Light), C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float,
                                     C.c_void_p, C.c_void_p]
    lib.oracle_connect_vertices.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_float, C.c_void_p]
    lib.oracle_connect_camera.argtypes = [C.POINTER(abi.Camera), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                          C.c_uint32, C.c_float, C.c_void_p]
    lib.oracle_sincos2pi.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.oracle_half_round.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.oracle_area_exclude.restype = C.c_int
    lib.oracle_area_exclude.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    lib.oracle_area_light_info.argtypes = [C.c_void_p, C.POINTER(abi.AreaLightInfo)]
    lib.oracle_area_table.restype = C.c_uint32
    lib.oracle_area_table.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.oracle_area_light_sample.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.oracle_bmfr_create.restype = C.c_void_p
    lib.oracle_bmfr_create.argtypes = [C.c_uint32, C.c_uint32]
    lib.oracle_bmfr_destroy.argtypes = [C.c_void_p]
    lib.oracle_bmfr_reset.argtypes = [C.c_void_p]
    lib.oracle_bmfr_execute.restype = C.c_int
    lib.oracle_bmfr_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.oracle_bmfr_execute.argtypes = [C.c_void_p, C.POINTER(abi.BmfrParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.oracle_bmfr_execute_motion.restype = C.c_int
    lib.oracle_bmfr_execute_motion.argtypes = [C.c_void_p, C.POINTER(abi.BmfrParams)] + [C.c_void_p] * 5
    _lib = lib
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _records(a, width):
    a = np.ascontiguousarray(a, np.float32)
    assert a.ndim == 2 and a.shape[1] == width
    return a


def light_nee(abi, lights, surfaces, seeds, mat_index, min_t):
    """oracle_light_nee: lights a ctypes array of abi.Light, surfaces (n, 24) float32, seeds (n,) uint32.
    -> (samples (n, 12) float32 in the bdpt_light_sample layout, the states after the selection draw)"""
    lib = load_oracle(abi)
    surfaces, seeds = _records(surfaces, 24), np.ascontiguousarray(seeds, np.uint32)
    out, after = np.zeros((len(seeds), 12), np.float32), np.zeros(len(seeds), np.uint32)
    lib.oracle_light_nee(lights, len(lights), _p(surfaces), _p(seeds), len(seeds), mat_index, min_t, _p(out), _p(after))
    return out, after


def connect_vertices(abi, eye, light, mat_index, min_t, eye_prev=None, light_prev=None, eye_specular=None, light_specular=None):
    """oracle_connect_vertices -> (n, 12) float32 in the bdpt_connect_sample layout"""
    lib = load_oracle(abi)
    eye, light = _records(eye, 24), _records(light, 24)
    opt = [None if a is None else np.ascontiguousarray(a, t) for a, t in
           ((eye_prev, np.float32), (light_prev, np.float32), (eye_specular, np.uint8), (light_specular, np.uint8))]
    out = np.zeros((len(eye), 12), np.float32)
    lib.oracle_connect_vertices(_p(eye), _p(light), *[None if a is None else _p(a) for a in opt], len(eye), mat_index, min_t, _p(out))
    return out


def connect_camera(abi, cam, width, height, jitter, light, mat_index, min_t, light_specular=None):
    """oracle_connect_camera -> (n, 16) float32 in the bdpt_camera_sample layout"""
    lib = load_oracle(abi)
    light = _records(light, 24)
    spec = None if light_specular is None else np.ascontiguousarray(light_specular, np.uint8)
    jit = np.array(jitter, np.float32)
    out = np.zeros((len(light), 16), np.float32)
    lib.oracle_connect_camera(C.byref(cam), width, height, _p(jit), _p(light), None if spec is None else _p(spec), len(light), mat_index,
                              min_t, _p(out))
    return out


def shade_hits(abi, scene, rays, hits, flags):
    """oracle_shade_hits: rays (n, 8) float32 (bdpt_ray), hits (n, 4) float32 (bdpt_hit: t, u, v, prim bits) -> (n, 24) float32
    in the bdpt_surface layout"""
    lib = load_oracle(abi)
    rays, hits = _records(rays, 8), _records(hits, 4)
    out = np.zeros((len(hits), 24), np.float32)
    lib.oracle_shade_hits(scene, _p(rays), _p(hits), len(hits), flags, _p(out))
    return out


def alpha_test(abi, scene, prim, uv):
    """oracle_alpha_test: prim (n,) uint32, uv (n, 2) float32 barycentrics -> (n,) bool, True where the candidate is ignored"""
    lib = load_oracle(abi)
    prim, uv = np.ascontiguousarray(prim, np.uint32), _records(uv, 2)
    fails = np.zeros(len(prim), np.uint8)
    lib.oracle_alpha_test(scene, _p(prim), _p(uv), len(prim), _p(fails))
    return fails != 0


class OracleRender:
    """Full-frame host buffers + the three oracle passes, mirroring the product's frame loop."""

    def __init__(self, abi, scene_desc, width, height, y0=0, y1=None):
        self.abi = abi
        self.lib = load_oracle(abi)
        self.scene = self.lib.oracle_scene_create(C.byref(scene_desc))
        assert self.scene, "oracle_scene_create failed"
        self.W, self.H = width, height
        self.y0, self.y1 = y0, height if y1 is None else y1
        n = width * height
        self.chan = {k: np.zeros((n, 4), np.float32) for k in
                     ("worldPosition", "worldNormal", "materialDiffuse", "materialSpecRough", "materialExtra",
                      "emissive", "out")}
        self.splat = np.zeros((n, 4), np.uint64)
        self.frame = OracleFrame(width, height, self.y0, self.y1, _p(self.chan["worldPosition"]),
                                 _p(self.chan["worldNormal"]), _p(self.chan["materialDiffuse"]),
                                 _p(self.chan["materialSpecRough"]), _p(self.chan["materialExtra"]),
                                 _p(self.chan["emissive"]), _p(self.chan["out"]), _p(self.splat))

    def close(self):
        if self.scene:
            self.lib.oracle_scene_destroy(self.scene)
            self.scene = None

    def set_environment(self, env_map=None, color=(0.0, 0.0, 0.0, 0.0)):
        """env_map: float32 [h, w, 4] host array (lat-long) or None for the constant colour."""
        e = self.abi.Environment()
        if env_map is not None:
            self._env_keep = np.ascontiguousarray(env_map, np.float32)
            e.envMap = self._env_keep.ctypes.data
            e.height, e.width = self._env_keep.shape[0], self._env_keep.shape[1]
        for i in range(4):
            e.color[i] = float(color[i])
        self.lib.oracle_set_environment(self.scene, C.byref(e))

    def gbuffer(self, cam, gparams, env=None, flags=0, threads=8):
        rc = self.lib.oracle_gbuffer(self.scene, C.byref(cam), C.byref(gparams), _p(env) if env is not None else None,
                                     C.byref(self.frame), flags, threads)
        assert rc == 0

    def bdpt(self, cam, params, flags=0, threads=8, zero_splat=True):
        if zero_splat:
            self.splat[:] = 0
        cnt = self.abi.Counters()
        rc = self.lib.oracle_bdpt(self.scene, C.byref(cam), C.byref(params), C.byref(self.frame), flags, threads,
                                  C.byref(cnt))
        assert rc == 0, rc
        return cnt

    def resolve(self):
        assert self.lib.oracle_resolve(C.byref(self.frame)) == 0

    def image(self):
        return self.chan["out"].reshape(self.H, self.W, 4)


class OracleBmfr:
    """The denoise pass of oracle/bmfr_oracle.cpp with its own history, mirroring bdpt_bmfr_execute."""

    def __init__(self, abi, width, height):
        self.lib = load_oracle(abi)
        self.h = self.lib.oracle_bmfr_create(width, height)
        self.W, self.H = width, height

    def reset(self):
        self.lib.oracle_bmfr_reset(self.h)

    def execute(self, params, cur_pos, cur_norm, albedo, noisy, prev_pos=None):
        """All arrays float32 [H*W, 4], C-contiguous; `noisy` is updated in place.  prev_pos: bdpt_bmfr_execute_motion's
        channel."""
        for a in (cur_pos, cur_norm, albedo, noisy) + (() if prev_pos is None else (prev_pos,)):
            assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"] and a.size == self.W * self.H * 4
        rc = self.lib.oracle_bmfr_execute_motion(self.h, C.byref(params), _p(cur_pos), _p(cur_norm), _p(albedo),
                                                 None if prev_pos is None else _p(prev_pos), _p(noisy))
        assert rc == 0
        return noisy

    def state(self):
        """(prev_noisy [n,4], accept [n], prev_pixel [n,2]): what the last execute left for the next one."""
        n = self.W * self.H
        noisy, accept, pixel = np.zeros((n, 4), np.float32), np.zeros(n, np.uint32), np.zeros((n, 2), np.float32)
        self.lib.oracle_bmfr_state(self.h, _p(noisy), _p(accept), _p(pixel))
        return noisy, accept, pixel

    def close(self):
        if self.h:
            self.lib.oracle_bmfr_destroy(self.h)
            self.h = None
