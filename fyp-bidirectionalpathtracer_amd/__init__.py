"""MI355X-native bidirectional path-tracing render pass — Python plumbing over the C ABI.

The product is ``csrc/libbdpt_amd.so`` (HIP kernels for gfx950 behind ``include/bdpt.h``) and
the C++ host mirror under ``host/``.  This module only provides what tests and ``bench.py``
need: ctypes bindings, torch tensors as device memory for the ResourceManager channels, HIP
streams, and the per-frame calling sequence of the reference pipeline
(SharedUtils/RenderingPipeline.cpp:666-682: G-buffer pass -> BDPT pass -> accumulation pass).
There is no CPU fallback anywhere in this package.
"""
import ctypes as C

from . import abi, tiling
from .abi import (Camera, Counters, GBuffer, GBufferParams, Params, SceneDesc, Stripes, Tile, TileInfo, load_library)

__all__ = ["abi", "tiling", "Scene", "Context", "FramePipeline", "load_library", "source_hash", "ADAPTIVE_DEFAULTS",
           "adaptive_params"]

# Channel names of the reference's ResourceManager (BDPTPass.cpp:27-29, LightProbeGBufferPass.cpp:46-51)
GBUFFER_CHANNELS = ("WorldPosition", "WorldNormal", "MaterialDiffuse", "MaterialSpecRough", "MaterialExtraParams",
                    "Emissive")
OUTPUT_CHANNEL = "PipelineOutput"  # ResourceManager::kOutputChannel, SharedUtils/ResourceManager.cpp:22
AO_CHANNEL = "AmbientOcclusion"  # the channel FramePipeline.ambient_occlusion and bdpt_render --ao write
GI_CHANNEL = "DiffuseGI"  # the channel FramePipeline.diffuse_gi and bdpt_render --gi write
DIRECT_CHANNEL = "DirectLighting"  # the channel FramePipeline.direct_lighting and bdpt_render --direct write
SKY_CHANNEL = "SkyLighting"  # the channel FramePipeline.sky_lighting and bdpt_render --sky write
RIS_CHANNEL = "ResampledDirect"  # the channel FramePipeline.ris_lighting and bdpt_render --ris write
RESTIR_CHANNEL = "RestirDirect"  # the channel FramePipeline.restir_lighting writes


class BdptError(RuntimeError):
    pass


def source_hash():
    """SHA-256 over the sources libbdpt_amd.so is built from — exactly the Makefile's prerequisites: csrc/*.{hip,hpp,h,cpp},
    the host files linked into it (host/Scene.cpp, Atrium.cpp, SceneLoader.cpp, ImageDecode.cpp: the scene generators and
    the loader shape the measured workload), host/Scene.h, include/*.h and the Makefile.  Ties hardware-counter files
    (profiles/<round>/roofline_pmc.json) to the build they were measured on."""
    import glob
    import hashlib
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    files = sorted(glob.glob(os.path.join(here, "csrc", "*.hip")) + glob.glob(os.path.join(here, "csrc", "*.hpp")) +
                   glob.glob(os.path.join(here, "csrc", "*.h")) + glob.glob(os.path.join(here, "csrc", "*.cpp")) +
                   [os.path.join(here, "csrc", "Makefile")] +
                   [os.path.join(here, "host", f) for f in ("Scene.cpp", "Atrium.cpp", "SceneLoader.cpp", "ImageDecode.cpp")] +
                   [os.path.join(here, "host", "Scene.h")] + glob.glob(os.path.join(root, "include", "*.h")))
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.relpath(f, root).encode() + b"\0")
        h.update(open(f, "rb").read())
    return h.hexdigest()


class Scene:
    """Host scene container (include/bdpt_scene.h)."""

    def __init__(self, handle):
        self._lib = load_library()
        if not handle:
            raise BdptError("scene creation failed")
        self._h = C.c_void_p(handle)
        self.desc = SceneDesc()
        if self._lib.bdpt_scene_get_desc(self._h, C.byref(self.desc)) != 0:
            raise BdptError("bdpt_scene_get_desc failed")

    @classmethod
    def cornell(cls):
        return cls(load_library().bdpt_scene_create_cornell())

    @classmethod
    def atrium(cls, seed=1, target_triangles=262144):
        return cls(load_library().bdpt_scene_create_atrium(seed, target_triangles))

    @classmethod
    def atrium_uneven(cls, seed=1, target_triangles=262144):
        """The atrium with heavy-tailed triangle areas (two-triangle walls and floors beside finely tessellated ornaments)."""
        return cls(load_library().bdpt_scene_create_atrium_uneven(seed, target_triangles))

    @classmethod
    def courtyard(cls, seed=1, target_triangles=262144, foliage_fraction=0.5):
        """Atrium + alpha-masked foliage (San Miguel stand-in, BASELINE config 5)."""
        return cls(load_library().bdpt_scene_create_courtyard(seed, target_triangles, foliage_fraction))

    @classmethod
    def soup(cls, seed, num_triangles, max_edge=0.25):
        return cls(load_library().bdpt_scene_create_soup(seed, num_triangles, max_edge))

    @classmethod
    def load(cls, path, threads=None):
        """`.fscene` / `.obj` ingestion (SharedUtils/SceneLoaderWrapper.cpp:56-103).  `threads`: host threads of the model
        loader for this call (None: the default; the scene does not depend on it)."""
        msg = C.create_string_buffer(512)
        lib = load_library()
        before = lib.bdpt_scene_load_threads(int(threads)) if threads is not None else None
        try:
            h = lib.bdpt_scene_load(str(path).encode(), msg, 512)
        finally:
            if before is not None:
                lib.bdpt_scene_load_threads(before)
        if not h:
            raise BdptError("bdpt_scene_load: " + msg.value.decode(errors="replace"))
        return cls(h)

    def camera(self, aspect):
        cam = Camera()
        if self._lib.bdpt_scene_get_camera(self._h, float(aspect), C.byref(cam)) != 0:
            raise BdptError("bdpt_scene_get_camera failed")
        return cam

    def close(self):
        if self._h:
            self._lib.bdpt_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def camera_view_proj(pos, target, up, focal_length_mm=21.0, frame_height_mm=24.0, aspect=1.7777, near=0.1, far=1000.0):
    """Falcor's jitter-free viewProjMat, row-major (Camera.cpp:60-105) -> 16 floats for BmfrParams.prevViewProj."""
    out = (C.c_float * 16)()
    v3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    rc = load_library().bdpt_camera_view_proj(v3(pos), v3(target), v3(up), focal_length_mm, frame_height_mm, aspect,
                                              near, far, out)
    if rc != 0:
        raise BdptError("bdpt_camera_view_proj failed")
    return list(out)


def view_proj_of_camera(cam, near=0.1, far=1000.0):
    """camera_view_proj for an abi.Camera as bdpt_camera_look_at makes it: looking along cameraW with cameraV up,
    tan(fovY / 2) = |cameraV| / |cameraW|, aspect = |cameraU| / |cameraV|."""
    import math
    length = lambda v: math.sqrt(sum(float(x) * float(x) for x in v))
    pos = [float(x) for x in cam.posW]
    u, v, w = length(cam.cameraU), length(cam.cameraV), length(cam.cameraW)
    return camera_view_proj(pos, [pos[i] + float(cam.cameraW[i]) for i in range(3)], list(cam.cameraV), 12.0 * w / v, 24.0, u / v,
                            near, far)


def msaa_jitter(counter_before_increment):
    j = (C.c_float * 2)()
    load_library().bdpt_msaa_jitter(counter_before_increment & 0xFFFFFFFF, j)
    return float(j[0]), float(j[1])


def ao_default_radius(scene_desc):
    """The AO pass's radius for a newly loaded scene, max(0.1, scene radius * 0.05) (CommonPasses/AmbientOcclusionPass.cpp:62),
    with the scene radius half the length of the bounding box's half extent (Falcor Graphics/Scene/Scene.cpp:92, Utils/AABB.h:113),
    in fp32 as the host's Scene::getRadius computes it."""
    import numpy as np
    f = np.float32
    p = np.ctypeslib.as_array(scene_desc.positions, (int(scene_desc.numVertices), 3))
    e = (p.max(axis=0).astype(f) - p.min(axis=0).astype(f)) * f(0.5)
    radius = np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2], dtype=f) * f(0.5)
    return float(max(f(0.1), radius * f(0.05)))


def keep_for_stream(stream, arrays):
    """GPU tensors read by work enqueued on `stream` (an update): tell torch's caching allocator, which otherwise only
    orders a block's reuse after the stream that allocated it (Tensor.record_stream).  Not while capturing a graph: the
    tensors a graph reads are the caller's to keep for as long as the graph is replayed."""
    import torch
    if torch.cuda.is_current_stream_capturing():
        return
    for a in arrays:
        if a is not None and getattr(a, "is_cuda", False):
            a.record_stream(stream)


_TRACE_MODES = {"closest": abi.TRACE_CLOSEST, "closest_cull_back": abi.TRACE_CLOSEST_CULL_BACK, "any": abi.TRACE_ANY}


def _host_to_device(array, device):
    """A host array's device copy (Context.trace_rays' host path)."""
    import torch
    return torch.from_numpy(array).to(device)


class Context:
    """One bdpt_ctx = one GPU (one ctx per GPU, not thread-safe)."""

    # set_environment calls made through this object, and the count at the last env_prepare: FramePipeline.sky_lighting
    # prepares again when they differ.  Only calls are counted: a map rewritten in place is the caller's to prepare again.
    _env_serial = 0
    _env_prepared = None

    def __init__(self, device=0):
        self._lib = load_library()
        h = C.c_void_p()
        rc = self._lib.bdpt_create(int(device), C.byref(h))
        if rc != 0:
            raise BdptError(f"bdpt_create(device={device}) failed with {rc}: no usable HIP device — "
                            "the render pass has no CPU fallback")
        self._h = h
        self.device = device

    def _check(self, rc, what):
        if rc < 0:
            raise BdptError(f"{what} failed ({rc}): {self._lib.bdpt_last_error(self._h).decode()}")
        return rc

    def set_scene(self, desc):
        self._check(self._lib.bdpt_set_scene(self._h, C.byref(desc)), "bdpt_set_scene")

    def bvh_info(self):
        info = abi.BvhInfo()
        self._check(self._lib.bdpt_get_bvh_info(self._h, C.byref(info)), "bdpt_get_bvh_info")
        return info

    def set_camera(self, cam):
        self._check(self._lib.bdpt_set_camera(self._h, C.byref(cam)), "bdpt_set_camera")

    def _update_inputs(self, what, names, arrays):
        """(memory, pointers, sizes, keep) of an update's optional arrays: GPU torch tensors as they are, numpy arrays and
        CPU tensors as contiguous float32 copies, which `keep` holds until the call has returned.  `names` lists the
        arguments for the message of a mixture."""
        given = [a for a in arrays if a is not None]
        on_gpu = [bool(getattr(a, "is_cuda", False)) for a in given]
        if any(on_gpu):
            if not all(on_gpu):
                every = "both" if len(arrays) == 2 else "all"
                raise BdptError(f"{what}: {names} must {every} be GPU tensors or {every} host arrays")
            for a in given:
                if a.device.index != self.device:
                    raise BdptError(f"{what}: a tensor on {a.device} for the context of device {self.device}")
                if not a.is_contiguous() or str(a.dtype) != "torch.float32":
                    raise BdptError(f"{what}: device inputs must be contiguous float32 tensors")
            return (abi.MEMORY_DEVICE, [None if a is None else a.data_ptr() for a in arrays],
                    [None if a is None else a.numel() for a in arrays], arrays)
        import numpy as np
        # (a CPU torch tensor is host memory: its numpy view, never its address as a device pointer)
        keep = [None if a is None else np.ascontiguousarray(a.detach().numpy() if hasattr(a, "detach") else a, np.float32).reshape(-1)
                for a in arrays]
        return abi.MEMORY_HOST, [None if a is None else a.ctypes.data for a in keep], [None if a is None else a.size for a in keep], keep

    def update_geometry(self, positions, normals=None, bitangents=None, stream=None, keep_light_maps=False):
        """bdpt_update_geometry: new vertex positions (and normals / bitangents) for the scene, the tree refitted in place.
        GPU torch tensors take the device path: all of them must be contiguous float32 tensors on this context's device,
        and they must stay alive until the stream reaches the update (FramePipeline / TileRenderer see to that).  numpy
        arrays and CPU torch tensors take the host path: checked for finiteness and copied before this returns.  All
        arrays are numVertices x 3 float32.  Nothing is enqueued when an argument is refused."""
        u = abi.GeometryUpdate()
        u.memory, ptrs, sizes, _keep = self._update_inputs("update_geometry", "positions, normals and bitangents", [positions, normals, bitangents])
        n = sizes[0] // 3
        if sizes[0] != 3 * n or any(m is not None and m != 3 * n for m in sizes[1:]):
            raise BdptError("update_geometry: positions, normals and bitangents must be numVertices x 3 each")
        u.positions, u.normals, u.bitangents = ptrs
        u.numVertices = int(n)
        u.flags = abi.UPDATE_KEEP_LIGHT_MAPS if keep_light_maps else 0
        self._check(self._lib.bdpt_update_geometry(self._h, C.byref(u), stream), "bdpt_update_geometry")

    def set_skin(self, positions, bone_weights, bone_ids, num_bones, normals=None, bitangents=None):
        """bdpt_set_skin: the rest pose (numVertices x 3 float32 each; normals / bitangents optional), four weights
        (float32) and four bone ids (uint16) per vertex, all host arrays, copied before this returns.  Synchronises and
        allocates; not inside a stream capture.  positions=None drops the skin."""
        if positions is None:
            self._check(self._lib.bdpt_set_skin(self._h, None), "bdpt_set_skin")
            return
        import numpy as np

        def host(a, dtype):
            return None if a is None else np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype).reshape(-1)

        p, n, b, w = (host(a, np.float32) for a in (positions, normals, bitangents, bone_weights))
        ids = host(bone_ids, np.uint16)
        nv = p.size // 3
        if p.size != 3 * nv or any(a is not None and a.size != 3 * nv for a in (n, b)) or w.size != 4 * nv or ids.size != 4 * nv:
            raise BdptError("set_skin: positions, normals and bitangents must be numVertices x 3, weights and ids numVertices x 4")
        d = abi.SkinDesc()
        d.numVertices, d.numBones = int(nv), int(num_bones)
        d.positions, d.boneWeights, d.boneIds = p.ctypes.data, w.ctypes.data, ids.ctypes.data
        d.normals = None if n is None else n.ctypes.data
        d.bitangents = None if b is None else b.ctypes.data
        self._check(self._lib.bdpt_set_skin(self._h, C.byref(d)), "bdpt_set_skin")
        self._skin_vertices = int(nv)

    def update_skinned(self, bones, normal_bones=None, stream=None, keep_light_maps=False):
        """bdpt_update_skinned: the frame's bone matrices (numBones x 16 float32, m[4r+c], translation in floats 12..14;
        normal_bones: their inverse transposes, required iff the skin has normals); the vertices are skinned on the device
        and the tree refitted.  GPU torch tensors take the device path and numpy arrays / CPU tensors the host path, by
        the rules of update_geometry.  Nothing is enqueued when an argument is refused."""
        u = abi.SkinUpdate()
        u.memory, ptrs, sizes, _keep = self._update_inputs("update_skinned", "bones and normal_bones", [bones, normal_bones])
        n = sizes[0] // 16
        if sizes[0] != 16 * n or (sizes[1] is not None and sizes[1] != 16 * n):
            raise BdptError("update_skinned: bones and normal_bones must be numBones x 16 each")
        u.bones, u.normalBones = ptrs
        u.numBones = int(n)
        u.flags = abi.UPDATE_KEEP_LIGHT_MAPS if keep_light_maps else 0
        self._check(self._lib.bdpt_update_skinned(self._h, C.byref(u), stream), "bdpt_update_skinned")

    def skinned_buffers(self):
        """bdpt_skinned_buffers: the device addresses (int, or None for a stream the skin lacks) of the skinned positions,
        normals and bitangents; valid until set_skin / set_scene."""
        p, n, b = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self._lib.bdpt_skinned_buffers(self._h, C.byref(p), C.byref(n), C.byref(b)), "bdpt_skinned_buffers")
        return p.value, n.value, b.value

    def test_skin_kernel(self, path=abi.SKIN_PATH_AUTO, stream=None):
        """Test hook bdpt_test_skin_kernel: the skinning kernel alone, with the palette the last host-bone update_skinned
        staged; path SKIN_PATH_AUTO / _GLOBAL / _LDS."""
        self._check(self._lib.bdpt_test_skin_kernel(self._h, int(path), stream), "bdpt_test_skin_kernel")

    def read_skinned(self, stream=None):
        """The skinned streams copied to the host (numVertices x 3 float32 each, None for a stream the skin lacks); waits
        for `stream`."""
        return self._read_streams("read_skinned", self.skinned_buffers, "_skin_vertices", stream)

    def _read_streams(self, what, buffers, vertices, stream):
        """read_skinned / read_morphed: the device streams `buffers()` names copied to the host, getattr(self, vertices)
        x 3 float32 each; waits for `stream`."""
        import numpy as np
        self.sync(stream)
        nv = getattr(self, vertices)
        hip = C.CDLL("libamdhip64.so")
        out = []
        for ptr in buffers():
            if ptr is None:
                out.append(None)
                continue
            a = np.empty((nv, 3), np.float32)
            if hip.hipMemcpy(C.c_void_p(a.ctypes.data), C.c_void_p(ptr), C.c_size_t(a.nbytes), 2) != 0:
                raise BdptError(f"{what}: hipMemcpy failed")
            out.append(a)
        return tuple(out)

    def set_morph(self, target_start, vertex, d_positions, d_normals=None, d_bitangents=None, positions=None, normals=None,
                  bitangents=None):
        """bdpt_set_morph: morph targets as sparse deltas, all host arrays, copied before this returns.  target_start
        (numTargets + 1, uint32): target t owns entries [target_start[t], target_start[t + 1]); vertex (uint32, per
        entry, strictly ascending inside a target); d_positions / d_normals / d_bitangents: entries x 3 float32.
        positions / normals / bitangents: the base pose (numVertices x 3), for a context without a skin only (with a skin
        the base is its rest pose).  Synchronises and allocates; not inside a stream capture.  target_start=None drops
        the morph."""
        if target_start is None:
            self._check(self._lib.bdpt_set_morph(self._h, None), "bdpt_set_morph")
            return
        import numpy as np

        def host(a, dtype):
            return None if a is None else np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype).reshape(-1)

        ts, vx = host(target_start, np.uint32), host(vertex, np.uint32)
        dp, dn, db, p, n, b = (host(a, np.float32) for a in (d_positions, d_normals, d_bitangents, positions, normals, bitangents))
        if ts.size < 2 or vx is None or dp is None or int(ts[-1]) != vx.size or any(a is not None and a.size != 3 * vx.size for a in (dp, dn, db)):
            raise BdptError("set_morph: target_start must hold numTargets + 1 offsets ending at the entry count, vertex one id per "
                            "entry, the deltas entries x 3 each")
        given = [a for a in (p, n, b) if a is not None]
        if any(a.size % 3 or a.size != given[0].size for a in given) or (given and p is None):
            raise BdptError("set_morph: positions, normals and bitangents must be numVertices x 3 each, and positions among them")
        d = abi.MorphDesc()
        nv = p.size // 3 if p is not None else getattr(self, "_skin_vertices", 0)
        d.numVertices, d.numTargets = int(nv), int(ts.size - 1)
        d.targetStart, d.vertex = ts.ctypes.data, vx.ctypes.data
        for field, a in (("dPositions", dp), ("dNormals", dn), ("dBitangents", db), ("positions", p), ("normals", n), ("bitangents", b)):
            setattr(d, field, None if a is None else a.ctypes.data)
        self._check(self._lib.bdpt_set_morph(self._h, C.byref(d)), "bdpt_set_morph")
        self._morph_vertices = int(nv)

    def update_morphed(self, weights, bones=None, normal_bones=None, stream=None, keep_light_maps=False):
        """bdpt_update_morphed: the frame's morph weights (numTargets float32) and, for a context with a skin, its bone
        matrices (as update_skinned); the vertices are morphed and skinned on the device and the tree refitted.  GPU
        torch tensors take the device path and numpy arrays / CPU tensors the host path, by the rules of
        update_geometry, weights and palettes alike.  Nothing is enqueued when an argument is refused."""
        u = abi.MorphUpdate()
        if weights is None:
            raise BdptError("update_morphed: weights are required")
        u.memory, ptrs, sizes, _keep = self._update_inputs("update_morphed", "weights, bones and normal_bones", [weights, bones, normal_bones])
        nb = 0 if sizes[1] is None else sizes[1] // 16
        if sizes[0] == 0 or (sizes[1] is not None and sizes[1] != 16 * nb) or (sizes[2] is not None and sizes[2] != 16 * nb):
            raise BdptError("update_morphed: weights must be numTargets floats, bones and normal_bones numBones x 16 each "
                            "(normal_bones only with bones)")
        u.weights, u.bones, u.normalBones = ptrs
        u.numTargets, u.numBones = int(sizes[0]), int(nb)
        u.flags = abi.UPDATE_KEEP_LIGHT_MAPS if keep_light_maps else 0
        self._check(self._lib.bdpt_update_morphed(self._h, C.byref(u), stream), "bdpt_update_morphed")

    def morphed_buffers(self):
        """bdpt_morphed_buffers: the device addresses (int, or None for a stream the base lacks) of the positions, normals
        and bitangents a morphed update writes; valid until set_morph / set_skin / set_scene."""
        p, n, b = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self._lib.bdpt_morphed_buffers(self._h, C.byref(p), C.byref(n), C.byref(b)), "bdpt_morphed_buffers")
        return p.value, n.value, b.value

    def test_morph_kernel(self, path=abi.MORPH_PATH_AUTO, stream=None):
        """Test hook bdpt_test_morph_kernel: the morph kernel alone, with the weights and palettes the last host-pointer
        update_morphed staged; path MORPH_PATH_AUTO / _GLOBAL / _LDS."""
        self._check(self._lib.bdpt_test_morph_kernel(self._h, int(path), stream), "bdpt_test_morph_kernel")

    def read_morphed(self, stream=None):
        """The streams a morphed update writes copied to the host (numVertices x 3 float32 each, None for a stream the
        base lacks); waits for `stream`."""
        return self._read_streams("read_morphed", self.morphed_buffers, "_morph_vertices", stream)

    def trace_rays(self, rays, mode="closest", out=None, count=None, stream=None):
        """bdpt_trace_rays: closest-hit or any-hit queries of a batch of rays against the scene (semantics: include/bdpt.h
        "Ray queries").  `rays` is (N, 8) float32 in the bdpt_ray layout: origin xyz, tmin, direction xyz, tmax.
        `mode`: "closest", "closest_cull_back" or "any".

        GPU tensors (contiguous, on this context's device) are traced on `stream` without a synchronise: closest modes
        return (tuv, prim), float32 (N, 3) and int32 (N,) views of one (N, 4) bdpt_hit buffer; "any" returns uint8 (N,),
        1 = unoccluded.  `out` takes that buffer preallocated (closest modes: a contiguous (N, 4) float32 or int32 tensor;
        "any": a contiguous (N,) uint8 tensor), for graph capture.  `count` is a 1-element int32 / uint32 device tensor: only
        the first min(count, N) rays are traced, later outputs are left as they were.  The tensors must stay alive until
        the stream has reached the call (FramePipeline.trace_rays sees to that).

        numpy arrays and CPU tensors are copied to the device, traced, synchronised and returned as numpy arrays; no host
        address ever reaches the library.  Anything else is refused before the library is called."""
        import numpy as np
        import torch
        if mode not in _TRACE_MODES:
            raise BdptError(f"trace_rays: mode must be one of {sorted(_TRACE_MODES)}, not {mode!r}")
        closest = _TRACE_MODES[mode] != abi.TRACE_ANY

        def run(ptrs, n, cnt, res):
            d = abi.TraceDesc()
            d.rays, d.numRays, d.mode, d.numRaysDevice = ptrs[0], n, _TRACE_MODES[mode], cnt
            d.hits, d.visible = (res, None) if closest else (None, res)
            return self._lib.bdpt_trace_rays(self._h, C.byref(d), stream)

        res = self._surface_query("trace_rays", [("rays", rays, 8, (torch.float32,))],
                                  (4, (torch.float32, torch.int32)) if closest else (None, (torch.uint8,)), run, out, count,
                                  any_count_shape=True)
        if not closest:
            return res
        return res[:, :3], res.view(np.int32 if isinstance(res, np.ndarray) else torch.int32)[:, 3]

    # ---- surface queries (include/bdpt.h "Surface queries") ----
    def camera_rays(self, gparams, width, height, out=None, stream=None):
        """bdpt_camera_rays: the G-buffer pass's primary ray of every pixel of a width x height frame (pinhole or thin lens,
        jitter and frameCount of `gparams`, a GBufferParams), as an (width * height, 8) float32 GPU tensor in the bdpt_ray
        layout (origin xyz, tmin 0, direction xyz, tmax 1e38), row x + y * width.  `out` takes it preallocated (contiguous,
        float32, on this context's device).  Enqueued on `stream` without a synchronise."""
        import torch
        if not isinstance(gparams, abi.GBufferParams):
            raise BdptError("camera_rays: gparams must be a GBufferParams")
        w, h = int(width), int(height)
        if w <= 0 or h <= 0 or w * h >= 2**32:
            raise BdptError(f"camera_rays: bad frame size {w} x {h}")
        n = w * h
        if out is None:
            if not torch.cuda.is_available():
                raise BdptError("camera_rays: no GPU visible to torch (the queries have no CPU fallback)")
            out = torch.empty((n, 8), dtype=torch.float32, device=torch.device("cuda", self.device))
        else:
            self._check_gpu(out, "camera_rays", "out", (n, 8), (torch.float32,))
        self._check(self._lib.bdpt_camera_rays(self._h, C.byref(gparams), w, h, out.data_ptr(), stream), "bdpt_camera_rays")
        return out

    def shade_hits(self, rays, hits, normal_map=True, out=None, count=None, stream=None):
        """bdpt_shade_hits: the pass's shading at each hit, seen from its ray's origin.  `rays` (N, 8) float32 (bdpt_ray),
        `hits` (N, 4) float32 or int32 (bdpt_hit: t, u, v, prim bits — trace_rays' `out` buffer).  normal_map=True shades as
        the G-buffer pass does its primary hit, False as the walk does (no normal map).  Returns (N, 24) float32 in the
        bdpt_surface layout, columns
            0-2 posW, 3 dist, 4-6 N, 7 linearRoughness, 8-10 V, 11 IoR, 12-14 diffuse, 15 opacity,
            16-18 specular, 19 material (uint32 bits), 20-22 emissive, 23 prim (int32 bits, -1 = miss);
        read material and prim through .view(torch.int32) (numpy: .view(np.int32)).  GPU tensors, `out` and `count` as
        for trace_rays; host arrays are copied, shaded, synchronised and returned as numpy."""
        import torch
        f32, i32 = (torch.float32,), (torch.float32, torch.int32)
        flags = abi.SHADE_NORMAL_MAP if normal_map else 0

        def run(ptrs, n, cnt, res):
            d = abi.ShadeDesc()
            d.rays, d.hits, d.numHits, d.flags, d.numHitsDevice, d.surfaces = ptrs[0], ptrs[1], n, flags, cnt, res
            return self._lib.bdpt_shade_hits(self._h, C.byref(d), stream)

        return self._surface_query("shade_hits", [("rays", rays, 8, f32), ("hits", hits, 4, i32)], (24, i32), run, out, count)

    def keep_pose(self, stream=None):
        """bdpt_keep_pose: the current pose becomes the previous one (after prepare(motion=True)).  Once per frame, before
        that frame's updates — also in a frame without an update.  Enqueued on `stream` without a synchronise."""
        self._check(self._lib.bdpt_keep_pose(self._h, stream), "bdpt_keep_pose")

    def motion_query(self, hits, out=None, count=None, stream=None):
        """bdpt_motion_query: where each hit's surface point was in the previous pose.  `hits` (N, 4) float32 or int32
        (bdpt_hit: t, u, v, prim bits — trace_rays' `out` buffer).  Returns (N, 4) float32: (previous position, 1), zeros
        for a miss or a prim outside the scene.  GPU tensors, `out` and `count` as for trace_rays; host arrays are copied,
        queried, synchronised and returned as numpy."""
        import torch

        def run(ptrs, n, cnt, res):
            d = abi.MotionDesc()
            d.hits, d.num, d.reserved, d.numDevice, d.prevPositions = ptrs[0], n, 0, cnt, res
            return self._lib.bdpt_motion_query(self._h, C.byref(d), stream)

        return self._surface_query("motion_query", [("hits", hits, 4, (torch.float32, torch.int32))], (4, (torch.float32,)), run, out,
                                   count)

    def sample_bsdf(self, surfaces, seeds, mat_index=0, from_lobe=False, out=None, count=None, stream=None):
        """bdpt_bsdf_query(SAMPLE): sampleBRDF at each (N, 24) bdpt_surface record (shade_hits' output) with its seed
        ((N,) uint32 or int32 RNG states, read by value).  mat_index 0 GGX, 1 Lambertian; from_lobe sets
        BDPT_PARAM_SPECULAR_FROM_LOBE.  Returns (N, 8) float32 in the bdpt_bsdf_sample layout: 0-2 direction, 3 pdf,
        4-6 weight, 7 specular (uint32 bits, 1 = the specular lobe).  A miss record gives zeros."""
        import torch
        i32 = (torch.float32, torch.int32)
        mat, flags = self._bsdf_mode("sample_bsdf", mat_index, from_lobe)

        def run(ptrs, n, cnt, res):
            d = abi.BsdfDesc()
            d.surfaces, d.num, d.mode, d.numDevice, d.matIndex, d.flags = ptrs[0], n, abi.BSDF_SAMPLE, cnt, mat, flags
            d.seeds, d.samples = ptrs[1], res
            return self._lib.bdpt_bsdf_query(self._h, C.byref(d), stream)

        return self._surface_query("sample_bsdf", [("surfaces", surfaces, 24, i32), ("seeds", seeds, None, (torch.int32, torch.uint32))],
                                   (8, i32), run, out, count)

    def eval_bsdf(self, surfaces, dirs, mat_index=0, out=None, count=None, stream=None):
        """bdpt_bsdf_query(EVAL): evalBRDF at each (N, 24) bdpt_surface record toward dirs (N, 4) float32: L.xyz and w,
        w != 0 = evaluate the specular lobe (what sample_bsdf's column 7 says).  Returns (N, 4) float32: f.xyz, 0."""
        import torch
        f32, i32 = (torch.float32,), (torch.float32, torch.int32)
        mat, _ = self._bsdf_mode("eval_bsdf", mat_index, False)

        def run(ptrs, n, cnt, res):
            d = abi.BsdfDesc()
            d.surfaces, d.num, d.mode, d.numDevice, d.matIndex, d.flags = ptrs[0], n, abi.BSDF_EVAL, cnt, mat, 0
            d.dirs, d.values = ptrs[1], res
            return self._lib.bdpt_bsdf_query(self._h, C.byref(d), stream)

        return self._surface_query("eval_bsdf", [("surfaces", surfaces, 24, i32), ("dirs", dirs, 4, f32)], (4, f32), run, out, count)

    # ---- light queries (include/bdpt.h "Light queries") ----
    def sample_lights(self, surfaces, seeds, mat_index=0, min_t=1e-4, area_lights=False, use_hints=False, out=None,
                      seeds_out=None, compact=None, count=None, stream=None):
        """bdpt_light_query(NEE): one next-event sample of the pass per (N, 24) bdpt_surface record and seed ((N,) uint32 or
        int32 RNG states).  mat_index 0 GGX, 1 Lambertian; min_t is the rays' tmin; area_lights sets BDPT_PARAM_AREA_LIGHTS
        (the emitter table is one more light while it has weight), use_hints BDPT_LIGHT_USE_HINTS.  Returns (N, 12) float32
        in the bdpt_light_sample layout: 0-7 the shadow ray (bdpt_ray: origin, tmin, L, distance), 8-10 the unweighted,
        unclamped value of a visible light, 11 (through .view(torch.int32)) light | status << 16, status bit 0 = the value
        is non-zero, bit 1 = the occluder hint found the light occluded.  A miss record gives zeros.
        GPU tensors only: seeds_out (N,) takes the states after the selection draw (it may be `seeds`); compact = (rays (N, 8)
        float32, items (N,) int32 / uint32, count (1,) int32 / uint32, zeroed by the caller) takes the dense list of rays
        worth tracing, for trace_rays(rays, "any", count=count).  `out` and `count` as for the other queries."""
        import torch
        i32, u32 = (torch.float32, torch.int32), (torch.int32, torch.uint32)
        mat, _ = self._bsdf_mode("sample_lights", mat_index, False)
        flags = (abi.PARAM_AREA_LIGHTS if area_lights else 0) | (abi.LIGHT_USE_HINTS if use_hints else 0)
        extras = [("seeds_out", seeds_out, None, u32)]
        if compact is not None:
            if not isinstance(compact, (tuple, list)) or len(compact) != 3 or any(t is None for t in compact):
                raise BdptError("sample_lights: compact must be (rays, items, count), all three")
            extras += [("compact rays", compact[0], 8, (torch.float32,)), ("compact items", compact[1], None, u32),
                       ("compact count", compact[2], 1, u32)]
        else:
            compact = (None, None, None)

        def run(ptrs, n, cnt, res):
            d = abi.LightDesc()
            d.mode, d.num, d.numDevice, d.matIndex, d.flags, d.minT = abi.LIGHT_NEE, n, cnt, mat, flags, float(min_t)
            d.surfaces, d.seeds, d.samples = ptrs[0], ptrs[1], res
            d.seedsOut = None if seeds_out is None else seeds_out.data_ptr()
            d.compactRays, d.compactItems, d.compactCount = (None if t is None else t.data_ptr() for t in compact)
            return self._lib.bdpt_light_query(self._h, C.byref(d), stream)

        return self._surface_query("sample_lights", [("surfaces", surfaces, 24, i32), ("seeds", seeds, None, u32)], (12, i32), run,
                                   out, count, extras=extras, fn="bdpt_light_query")

    def emit_lights(self, seeds, min_t=1e-4, area_lights=False, out=None, seeds_out=None, count=None, stream=None):
        """bdpt_light_query(EMIT): the start of a light subpath of the pass (sampleLight) per seed ((N,) uint32 or int32 RNG
        states).  Returns (N, 12) float32 in the bdpt_light_emit layout: 0-7 the ray (bdpt_ray: the light's position or the
        point on an emitter, tmin = min_t, the sampled direction, 1e38), 8-10 the colour of light vertex 0, 11 the light
        (uint32 bits).  seeds_out (GPU tensor, (N,)) takes the states after all draws: the pass's seedL."""
        import torch
        i32, u32 = (torch.float32, torch.int32), (torch.int32, torch.uint32)
        flags = abi.PARAM_AREA_LIGHTS if area_lights else 0

        def run(ptrs, n, cnt, res):
            d = abi.LightDesc()
            d.mode, d.num, d.numDevice, d.matIndex, d.flags, d.minT = abi.LIGHT_EMIT, n, cnt, 0, flags, float(min_t)
            d.seeds, d.emits = ptrs[0], res
            d.seedsOut = None if seeds_out is None else seeds_out.data_ptr()
            return self._lib.bdpt_light_query(self._h, C.byref(d), stream)

        return self._surface_query("emit_lights", [("seeds", seeds, None, u32)], (12, i32), run, out, count,
                                   extras=[("seeds_out", seeds_out, None, u32)], fn="bdpt_light_query")

    # ---- connection queries (include/bdpt.h "Connection queries") ----
    @staticmethod
    def _compact_extras(what, compact):
        import torch
        u32 = (torch.int32, torch.uint32)
        if compact is None:
            return [], (None, None, None)
        if not isinstance(compact, (tuple, list)) or len(compact) != 3 or any(t is None for t in compact):
            raise BdptError(f"{what}: compact must be (rays, items, count), all three")
        return [("compact rays", compact[0], 8, (torch.float32,)), ("compact items", compact[1], None, u32),
                ("compact count", compact[2], 1, u32)], tuple(compact)

    def _gpu_only(self, what, tensors):
        for name, t in tensors:
            if t is not None and not getattr(t, "is_cuda", False):
                raise BdptError(f"{what}: {name} must be a GPU tensor on cuda:{self.device} (this query takes device memory only)")

    def connect_vertices(self, eye, light, mat_index=0, min_t=1e-4, eye_prev=None, light_prev=None, eye_specular=None,
                         light_specular=None, out=None, compact=None, count=None, stream=None):
        """bdpt_connect_query(VERTICES): eye vertex eye[i] against light vertex light[i], both (N, 24) bdpt_surface records
        (GPU tensors).  eye_prev / light_prev (N, 4) float32: the predecessors' positions (without them the records' V is the
        outgoing direction); eye_specular / light_specular (N,) uint8: the sampled lobe's specular flag (None = 0).  Returns
        (N, 12) float32 in the bdpt_connect_sample layout: 0-7 the connection ray (bdpt_ray), 8-10 (fsL * G) * fsE, unweighted
        and unclamped, 11 (through .view(torch.int32)) the status, bit 0 = the value is non-zero.  compact = (rays (N, 8)
        float32, items (N,), count (1,), zeroed by the caller) takes the dense list of the non-zero pairs' rays."""
        import torch
        i32, f32, u8 = (torch.float32, torch.int32), (torch.float32,), (torch.uint8,)
        mat, _ = self._bsdf_mode("connect_vertices", mat_index, False)
        self._gpu_only("connect_vertices", [("eye", eye), ("light", light)])
        extras = [("eye_prev", eye_prev, 4, f32), ("light_prev", light_prev, 4, f32), ("eye_specular", eye_specular, None, u8),
                  ("light_specular", light_specular, None, u8)]
        more, compact = self._compact_extras("connect_vertices", compact)

        def run(ptrs, n, cnt, res):
            d = abi.ConnectDesc()
            d.mode, d.num, d.numDevice, d.matIndex, d.minT = abi.CONNECT_VERTICES, n, cnt, mat, float(min_t)
            d.eye, d.light, d.samples = ptrs[0], ptrs[1], res
            d.eyePrev, d.lightPrev, d.eyeSpecular, d.lightSpecular = (None if t is None else t.data_ptr()
                                                                      for t in (eye_prev, light_prev, eye_specular, light_specular))
            d.compactRays, d.compactItems, d.compactCount = (None if t is None else t.data_ptr() for t in compact)
            return self._lib.bdpt_connect_query(self._h, C.byref(d), stream)

        return self._surface_query("connect_vertices", [("eye", eye, 24, i32), ("light", light, 24, i32)], (12, i32), run, out, count,
                                   extras=extras + more, fn="bdpt_connect_query")

    def connect_camera(self, light, width, height, pixel_jitter=(0.0, 0.0), mat_index=0, min_t=1e-4, light_specular=None,
                       out=None, compact=None, count=None, stream=None):
        """bdpt_connect_query(CAMERA): light vertex light[i] ((N, 24) bdpt_surface records, GPU tensor; V = the direction to
        the predecessor) against the context's camera for a width x height frame.  Returns (N, 16) float32 in the
        bdpt_camera_sample layout: 0-7 the ray to the camera (bdpt_ray), 8-10 f, 11 G, 12 the target pixel x + y * width and
        13 the status (both through .view(torch.int32); pixel -1 = none; status bit 1 = a pixel, bit 0 = f and G non-zero).
        compact as for connect_vertices: the rays of the items with a pixel."""
        import torch
        i32, u8 = (torch.float32, torch.int32), (torch.uint8,)
        mat, _ = self._bsdf_mode("connect_camera", mat_index, False)
        self._gpu_only("connect_camera", [("light", light)])
        w, h = int(width), int(height)
        if w <= 0 or h <= 0 or w * h >= 2**32:
            raise BdptError(f"connect_camera: bad frame size {w} x {h}")
        if len(pixel_jitter) != 2:
            raise BdptError("connect_camera: pixel_jitter must be two floats")
        more, compact = self._compact_extras("connect_camera", compact)

        def run(ptrs, n, cnt, res):
            d = abi.ConnectDesc()
            d.mode, d.num, d.numDevice, d.matIndex, d.minT = abi.CONNECT_CAMERA, n, cnt, mat, float(min_t)
            d.light, d.cameraSamples, d.width, d.height = ptrs[0], res, w, h
            d.pixelJitter[0], d.pixelJitter[1] = float(pixel_jitter[0]), float(pixel_jitter[1])
            d.lightSpecular = None if light_specular is None else light_specular.data_ptr()
            d.compactRays, d.compactItems, d.compactCount = (None if t is None else t.data_ptr() for t in compact)
            return self._lib.bdpt_connect_query(self._h, C.byref(d), stream)

        return self._surface_query("connect_camera", [("light", light, 24, i32)], (16, i32), run, out, count,
                                   extras=[("light_specular", light_specular, None, u8)] + more, fn="bdpt_connect_query")

    def splat_add(self, splat, pixels, values, visible=None, items=None, count=None, stream=None):
        """bdpt_splat_add: entry j adds values[k] ((M, 4) float32, xyz the clamped term) to pixel pixels[k] ((M,) int32 /
        uint32) of `splat`, k = items[j] ((n,) int32 / uint32) or j, when visible[j] ((n,) uint8) is non-zero or absent and
        the pixel is below numPixels.  `splat`: a contiguous GPU tensor of numPixels x 4 64-bit words ((P, 4) int64 / uint64),
        or the (pointer, number of 64-bit words) pair Context.splat_buffer() returns, for a whole-frame context's own
        buffer.  n = len(items) when given, else M; `count` (1,) caps it on the device.  GPU tensors only; nothing is
        returned."""
        import torch
        u32 = (torch.int32, torch.uint32)
        own = None
        if isinstance(splat, tuple):
            if len(splat) != 2 or not all(isinstance(v, int) and not isinstance(v, bool) for v in splat) or not splat[0] \
                    or splat[1] % 4 or splat[1] // 4 >= 2**32:
                raise BdptError("splat_add: a (pointer, words) splat must be what Context.splat_buffer() returns")
            own, splat = splat, None
        self._gpu_only("splat_add", [("splat", splat), ("pixels", pixels), ("values", values), ("visible", visible), ("items", items)])
        for name, t in (("splat", own if splat is None else splat), ("pixels", pixels), ("values", values)):
            if t is None:
                raise BdptError(f"splat_add: {name} is required")
        if pixels.dim() != 1:
            raise BdptError("splat_add: pixels must be (M,) int32/uint32")
        m = int(pixels.shape[0])
        self._check_gpu(pixels, "splat_add", "pixels", (m,), u32)
        self._check_gpu(values, "splat_add", "values", (m, 4), (torch.float32,))
        n = m
        if items is not None:
            if items.dim() != 1:
                raise BdptError("splat_add: items must be (n,) int32/uint32")
            n = int(items.shape[0])
            self._check_gpu(items, "splat_add", "items", (n,), u32)
        if visible is not None:
            self._check_gpu(visible, "splat_add", "visible", (n,), (torch.uint8,))
        if count is not None:
            self._check_gpu(count, "splat_add", "count", (1,), u32)
        if own is None:
            if splat.dim() != 2 or splat.shape[1] != 4 or splat.shape[0] >= 2**32:
                raise BdptError("splat_add: splat must be (numPixels, 4) int64/uint64")
            self._check_gpu(splat, "splat_add", "splat", tuple(splat.shape), (torch.int64, torch.uint64))
            own = (splat.data_ptr(), 4 * int(splat.shape[0]))
        d = abi.SplatDesc()
        d.num, d.numPixels = n, own[1] // 4
        d.numDevice = None if count is None else count.data_ptr()
        d.pixels, d.values, d.splat = pixels.data_ptr(), values.data_ptr(), own[0]
        d.visible = None if visible is None else visible.data_ptr()
        d.items = None if items is None else items.data_ptr()
        self._check(self._lib.bdpt_splat_add(self._h, C.byref(d), stream), "bdpt_splat_add")

    # ---- walk queries (include/bdpt.h "Walk queries") ----
    def walk(self, starts, seeds, steps, mat_index=0, min_t=1e-4, from_lobe=False, seed_per_step=False, first=None,
             first_specular=None, alive=None, out=None, samples=None, hits=None, count=None, stream=None):
        """bdpt_walk_query: one subpath per item, up to `steps` bounces (1 .. 16) in one launch — the loop trace_rays("closest")
        -> shade_hits(normal_map=False) -> sample_bsdf -> next ray, bit for bit.  GPU tensors only.
        starts (N, 12) float32 in the bdpt_walk_start layout, which is emit_lights' output: 0-7 the first ray (bdpt_ray; step 0
        takes its tmin and tmax, later steps min_t and 1e38), 8-10 the colour the walk starts with, 11 not read.  seeds (N,)
        uint32 / int32 RNG states, read by value at every step; with seed_per_step (steps, N), one state per step.
        first (N, 24) bdpt_surface records: the vertex the walk leaves (its position is the first ray's origin, and a ghost
        at step 0 copies it); first_specular (N,) uint8 its specular byte; alive (N,) uint8, 0 = the item has no path.
        Returns (vertices (steps, N, 24) float32 bdpt_surface records, info (steps, N, 4) float32: 0-2 the path colour at
        the vertex, 3 (through .view(torch.int32)) the status, abi.WALK_STATUS_STORED | _REAL | _SPECULAR); out= takes that
        pair preallocated.  samples (steps, N, 8) and hits (steps, N, 4), when given, take the sample drawn at each real
        vertex and the hit that made it.  `count` (1,) caps the items on the device; the plane stride stays N."""
        import torch
        f32, i32, u32, u8 = (torch.float32,), (torch.float32, torch.int32), (torch.int32, torch.uint32), (torch.uint8,)
        mat, flags = self._bsdf_mode("walk", mat_index, from_lobe)
        if isinstance(steps, bool) or not isinstance(steps, int) or not 1 <= steps <= abi.BDPT_MAX_DEPTH:
            raise BdptError(f"walk: steps must be an integer in 1 .. {abi.BDPT_MAX_DEPTH}, not {steps!r}")
        self._gpu_only("walk", [("starts", starts), ("seeds", seeds), ("first", first), ("first_specular", first_specular),
                                ("alive", alive), ("samples", samples), ("hits", hits), ("count", count)])
        if starts is None or seeds is None:
            raise BdptError("walk: starts and seeds are required")
        n = int(starts.shape[0]) if starts.dim() >= 1 else -1
        if n < 0 or steps * n >= 2**32:
            raise BdptError("walk: bad item count")
        self._check_gpu(starts, "walk", "starts", (n, 12), i32)
        self._check_gpu(seeds, "walk", "seeds", (steps, n) if seed_per_step else (n,), u32)
        for name, t, shape, dts in (("first", first, (n, 24), i32), ("first_specular", first_specular, (n,), u8),
                                    ("alive", alive, (n,), u8), ("samples", samples, (steps, n, 8), i32),
                                    ("hits", hits, (steps, n, 4), i32), ("count", count, (1,), u32)):
            if t is not None:
                self._check_gpu(t, "walk", name, shape, dts)
        if out is None:
            out = (torch.empty((steps, n, 24), dtype=torch.float32, device=starts.device),
                   torch.empty((steps, n, 4), dtype=torch.float32, device=starts.device))
        elif not isinstance(out, (tuple, list)) or len(out) != 2 or any(t is None for t in out):
            raise BdptError("walk: out must be (vertices, info), both")
        self._gpu_only("walk", [("out vertices", out[0]), ("out info", out[1])])
        self._check_gpu(out[0], "walk", "out vertices", (steps, n, 24), i32)
        self._check_gpu(out[1], "walk", "out info", (steps, n, 4), i32)
        d = abi.WalkDesc()
        d.num, d.steps, d.matIndex, d.minT = n, steps, mat, float(min_t)
        d.flags = flags | (abi.WALK_SEED_PER_STEP if seed_per_step else 0)
        d.starts, d.seeds, d.vertices, d.info = starts.data_ptr(), seeds.data_ptr(), out[0].data_ptr(), out[1].data_ptr()
        d.numDevice, d.first, d.firstSpecular, d.alive, d.samples, d.hits = (
            None if t is None else t.data_ptr() for t in (count, first, first_specular, alive, samples, hits))
        self._check(self._lib.bdpt_walk_query(self._h, C.byref(d), stream), "bdpt_walk_query")
        return tuple(t.view(torch.float32) if t.dtype == torch.int32 else t for t in out)

    # ---- ambient occlusion (include/bdpt.h "Ambient occlusion") ----
    @staticmethod
    def _ao_samples(what, samples):
        if isinstance(samples, bool) or not isinstance(samples, int) or not 1 <= samples <= abi.AO_MAX_SAMPLES:
            raise BdptError(f"{what}: samples must be an integer in 1 .. {abi.AO_MAX_SAMPLES}, not {samples!r}")
        return samples

    @staticmethod
    def _item_extras(alive, counts, seeds_out):
        """The optional GPU tensors of a per-item lighting query, as _surface_query's extras: alive (N,) uint8, counts and
        seeds_out (N,) 32-bit words."""
        import torch
        words = (torch.int32, torch.uint32)
        return [("alive", alive, None, (torch.uint8,)), ("counts", counts, None, words), ("seeds_out", seeds_out, None, words)]

    def ambient_occlusion(self, surfaces, seeds, samples, radius, min_t=1e-4, alive=None, out=None, counts=None, seeds_out=None,
                          count=None, stream=None):
        """bdpt_ao_query: `samples` (1 .. 64) cosine-weighted any-hit rays per (N, 24) bdpt_surface record (posW, N and prim
        are read) inside (min_t, radius), in one launch — the loop sample_bsdf(mat_index=1) -> rays -> trace_rays("any") ->
        count, bit for bit.  seeds (N,) uint32 / int32 RNG states; each sample takes two draws.  Returns (N,) float32: the
        share of unoccluded samples; a miss record (prim < 0), or an item whose `alive` byte is 0, gives 1 without a draw.
        GPU tensors only: alive (N,) uint8; counts (N,) takes the unoccluded samples (for exact accumulation over frames);
        seeds_out (N,) the states after 2 * samples draws (it may be `seeds`).  `out` and `count` as for the other queries."""
        import torch
        records, words = (torch.float32, torch.int32), (torch.int32, torch.uint32)  # the dtypes a record / a 32-bit word may have
        samples = self._ao_samples("ambient_occlusion", samples)
        extras = self._item_extras(alive, counts, seeds_out)

        def run(ptrs, n, cnt, res):
            d = abi.AoDesc()
            d.num, d.samples, d.numDevice, d.radius, d.minT = n, samples, cnt, float(radius), float(min_t)
            d.surfaces, d.seeds, d.ao = ptrs[0], ptrs[1], res
            d.alive, d.counts, d.seedsOut = (None if t is None else t.data_ptr() for t in (alive, counts, seeds_out))
            return self._lib.bdpt_ao_query(self._h, C.byref(d), stream)

        return self._surface_query("ambient_occlusion", [("surfaces", surfaces, 24, records), ("seeds", seeds, None, words)],
                                   (None, (torch.float32,)), run, out, count, extras=extras, fn="bdpt_ao_query")

    def ao_execute(self, params, gbuffer, out_ptr, stream=None):
        """bdpt_ao_execute: the reference's AO pass on the context's tile pixels — abi.AoParams (frameCount, radius, minT,
        samples), the full-frame G-buffer, and the full-frame RGBA32F image at `out_ptr`, which gets (ao, ao, ao, 1)."""
        self._check(self._lib.bdpt_ao_execute(self._h, C.byref(params), C.byref(gbuffer), out_ptr, stream), "bdpt_ao_execute")

    # ---- environment lighting (include/bdpt.h "Environment lighting") ----
    @staticmethod
    def _sky_samples(what, samples):
        if isinstance(samples, bool) or not isinstance(samples, int) or not 1 <= samples <= abi.SKY_MAX_SAMPLES:
            raise BdptError(f"{what}: samples must be an integer in 1 .. {abi.SKY_MAX_SAMPLES}, not {samples!r}")
        return samples

    def env_prepare(self, stream=None):
        """bdpt_env_prepare: build the sampling table of the map set_environment bound (the first call for a map size
        allocates: not inside a capture).  set_environment drops the table; the environment queries need it.  The table
        is a snapshot of the map's contents: a caller who rewrites the map in place (an animated probe) calls this again."""
        self._check(self._lib.bdpt_env_prepare(self._h, stream), "bdpt_env_prepare")
        self._env_prepared = self._env_serial

    def env_info(self):
        """bdpt_get_env_info (synchronises): abi.EnvInfo — width, height, total, max, the scan chunk sizes, the table's bytes
        and device addresses."""
        info = abi.EnvInfo()
        self._check(self._lib.bdpt_get_env_info(self._h, C.byref(info)), "bdpt_get_env_info")
        return info

    def env_table(self):
        """Test hook bdpt_test_env_table (synchronises): the table as numpy (cdf (H, W) uint32, rowCdf (H,) uint64)."""
        import numpy as np
        info = self.env_info()
        cdf, row = np.zeros((info.height, info.width), np.uint32), np.zeros(info.height, np.uint64)
        self._check(self._lib.bdpt_test_env_table(self._h, cdf.ctypes.data, row.ctypes.data), "bdpt_test_env_table")
        return cdf, row

    def env_sample(self, surfaces, seeds, mat_index=1, min_t=1e-4, out=None, seeds_out=None, compact=None, count=None, stream=None):
        """bdpt_env_query(SAMPLE): one importance sample of the environment map per (N, 24) bdpt_surface record and seed ((N,)
        uint32 / int32 RNG states; four draws each).  Returns (N, 20) float32 in the bdpt_env_sample layout: 0-7 the shadow
        ray (origin, tmin, direction, 1e38), 8-10 the texel's radiance, 11 the solid-angle pdf, 12-14 the unweighted,
        unclamped value of a visible environment (mat_index 1 Lambertian, 0 GGX), 15 the texel y * W + x and 16 the status
        (both through .view(torch.int32); status bit 0 = the value is non-zero).  A miss record gives zeros.  GPU tensors
        only: seeds_out (N,) takes the states after the four draws (it may be `seeds`); compact = (rays (N, 8) float32,
        items (N,), count (1,), zeroed by the caller) takes the dense list of the non-zero items' rays, for
        trace_rays(rays, "any", count=count).  `out` and `count` as for the other queries."""
        import torch
        i32, u32 = (torch.float32, torch.int32), (torch.int32, torch.uint32)
        mat, _ = self._bsdf_mode("env_sample", mat_index, False)
        more, compact = self._compact_extras("env_sample", compact)

        def run(ptrs, n, cnt, res):
            d = abi.EnvDesc()
            d.mode, d.num, d.numDevice, d.matIndex, d.minT = abi.ENV_SAMPLE, n, cnt, mat, float(min_t)
            d.surfaces, d.seeds, d.samples = ptrs[0], ptrs[1], res
            d.seedsOut = None if seeds_out is None else seeds_out.data_ptr()
            d.compactRays, d.compactItems, d.compactCount = (None if t is None else t.data_ptr() for t in compact)
            return self._lib.bdpt_env_query(self._h, C.byref(d), stream)

        return self._surface_query("env_sample", [("surfaces", surfaces, 24, i32), ("seeds", seeds, None, u32)], (20, i32), run, out,
                                   count, extras=[("seeds_out", seeds_out, None, u32)] + more, fn="bdpt_env_query")

    def env_eval(self, dirs, out=None, count=None, stream=None):
        """bdpt_env_query(EVAL): the environment toward (N, 4) float32 directions (xyz read), for MIS against env_sample.
        Returns (N, 8) float32 in the bdpt_env_eval layout: 0-2 the radiance (the G-buffer miss shader's lookup), 3 the
        sampler's solid-angle pdf, 4 (through .view(torch.int32)) the texel, -1 = outside the map."""
        import torch

        def run(ptrs, n, cnt, res):
            d = abi.EnvDesc()
            d.mode, d.num, d.numDevice, d.dirs, d.evals = abi.ENV_EVAL, n, cnt, ptrs[0], res
            return self._lib.bdpt_env_query(self._h, C.byref(d), stream)

        return self._surface_query("env_eval", [("dirs", dirs, 4, (torch.float32,))], (8, (torch.float32, torch.int32)), run, out, count,
                                   fn="bdpt_env_query")

    def sky_lighting(self, surfaces, seeds, samples, clamp=float(3.4028234663852886e38), min_t=1e-4, alive=None, out=None, counts=None,
                     seeds_out=None, count=None, stream=None):
        """bdpt_sky_query: `samples` (1 .. 64) importance-sampled any-hit rays toward the environment map per (N, 24)
        bdpt_surface record (posW, N, diffuse and prim are read), in one launch — the loop env_sample(mat_index=1) -> clamp ->
        trace_rays("any") on the non-zero terms -> ordered add, bit for bit.  seeds (N,) uint32 / int32 RNG states; each
        sample takes four draws.  `clamp` bounds every component of a sample's value.  Returns (N, 4) float32: (the mean of
        the visible terms, 1); a miss record (prim < 0), or an item whose `alive` byte is 0, gives (diffuse, 1) without a
        draw.  GPU tensors only: alive (N,) uint8; counts (N,) takes the samples traced and found unoccluded; seeds_out (N,)
        the states after 4 * samples draws (it may be `seeds`).  `out` and `count` as for the other queries."""
        import torch
        records, words = (torch.float32, torch.int32), (torch.int32, torch.uint32)
        samples = self._sky_samples("sky_lighting", samples)
        extras = self._item_extras(alive, counts, seeds_out)

        def run(ptrs, n, cnt, res):
            d = abi.SkyDesc()
            d.num, d.samples, d.numDevice, d.clampUpper, d.minT = n, samples, cnt, float(clamp), float(min_t)
            d.surfaces, d.seeds, d.color = ptrs[0], ptrs[1], res
            d.alive, d.counts, d.seedsOut = (None if t is None else t.data_ptr() for t in (alive, counts, seeds_out))
            return self._lib.bdpt_sky_query(self._h, C.byref(d), stream)

        return self._surface_query("sky_lighting", [("surfaces", surfaces, 24, records), ("seeds", seeds, None, words)],
                                   (4, (torch.float32,)), run, out, count, extras=extras, fn="bdpt_sky_query")

    def sky_execute(self, params, gbuffer, out_ptr, stream=None):
        """bdpt_sky_execute: sky lighting on the context's tile pixels — abi.SkyParams (frameCount, clampUpper, minT, samples),
        the full-frame G-buffer, and the full-frame RGBA32F image at `out_ptr`, which gets (colour, 1)."""
        self._check(self._lib.bdpt_sky_execute(self._h, C.byref(params), C.byref(gbuffer), out_ptr, stream), "bdpt_sky_execute")

    # ---- MIS sky lighting (include/bdpt.h "Environment lighting", DESIGN.md "MIS sky lighting") ----
    @staticmethod
    def _sky_techniques(what, techniques):
        if isinstance(techniques, bool) or not isinstance(techniques, int) or not 1 <= techniques <= 3:
            raise BdptError(f"{what}: techniques must be 1 (table samples), 2 (BSDF samples) or 3 (both), not {techniques!r}")
        return techniques

    def bsdf_pdf(self, surfaces, dirs, mat_index=0, out=None, count=None, stream=None):
        """bdpt_bsdf_pdf_query: the BSDF of each (N, 24) bdpt_surface record toward dirs (N, 4) float32 (xyz = L, used as
        given), for MIS.  Returns (N, 4) float32: 0-2 the unweighted BSDF times cosine that next-event estimation uses, 3 the
        solid-angle density with which sample_bsdf draws L (mat_index 0 GGX: the mixture of its two lobes; 1 Lambertian).  A
        miss record gives zeros."""
        import torch
        f32, i32 = (torch.float32,), (torch.float32, torch.int32)
        mat, _ = self._bsdf_mode("bsdf_pdf", mat_index, False)

        def run(ptrs, n, cnt, res):
            d = abi.BsdfPdfDesc()
            d.num, d.matIndex, d.numDevice, d.surfaces, d.dirs, d.values = n, mat, cnt, ptrs[0], ptrs[1], res
            return self._lib.bdpt_bsdf_pdf_query(self._h, C.byref(d), stream)

        return self._surface_query("bsdf_pdf", [("surfaces", surfaces, 24, i32), ("dirs", dirs, 4, f32)], (4, f32), run, out, count,
                                   fn="bdpt_bsdf_pdf_query")

    def sky_lighting_mis(self, surfaces, seeds, samples, mat_index=0, techniques=3, clamp=float(3.4028234663852886e38), min_t=1e-4,
                         alive=None, out=None, counts=None, seeds_out=None, count=None, stream=None):
        """bdpt_sky_mis_query: sky lighting with multiple importance sampling.  Per (N, 24) bdpt_surface record and sample
        one any-hit ray toward a direction drawn from the environment map's table (techniques bit 0) and one toward a
        direction drawn from the BSDF (bit 1; mat_index 0 GGX, 1 Lambertian), each weighted by the balance heuristic, in one
        launch — the loop env_sample -> bsdf_pdf -> sample_bsdf -> env_eval -> bsdf_pdf -> trace_rays("any") twice -> ordered
        adds, bit for bit.  With one technique it is the plain estimator.  seeds (N,) uint32 / int32 RNG states: four draws
        per table sample, three per BSDF sample.  `clamp` bounds every component of a term.  Returns (N, 4) float32: (the sum
        of the visible terms over `samples`, 1); a miss record, or an item whose `alive` byte is 0, gives (diffuse, 1) without
        a draw.  GPU tensors only: alive (N,) uint8; counts (N,) takes the terms traced and found unoccluded (0 .. 2 *
        samples); seeds_out (N,) the states after the draws (it may be `seeds`).  `out` and `count` as for the other queries."""
        import torch
        records, words = (torch.float32, torch.int32), (torch.int32, torch.uint32)
        samples = self._sky_samples("sky_lighting_mis", samples)
        mat, _ = self._bsdf_mode("sky_lighting_mis", mat_index, False)
        techniques = self._sky_techniques("sky_lighting_mis", techniques)
        extras = self._item_extras(alive, counts, seeds_out)

        def run(ptrs, n, cnt, res):
            d = abi.SkyMisDesc()
            d.num, d.samples, d.numDevice, d.clampUpper, d.minT = n, samples, cnt, float(clamp), float(min_t)
            d.matIndex, d.techniques = mat, techniques
            d.surfaces, d.seeds, d.color = ptrs[0], ptrs[1], res
            d.alive, d.counts, d.seedsOut = (None if t is None else t.data_ptr() for t in (alive, counts, seeds_out))
            return self._lib.bdpt_sky_mis_query(self._h, C.byref(d), stream)

        return self._surface_query("sky_lighting_mis", [("surfaces", surfaces, 24, records), ("seeds", seeds, None, words)],
                                   (4, (torch.float32,)), run, out, count, extras=extras, fn="bdpt_sky_mis_query")

    def sky_mis_execute(self, params, gbuffer, out_ptr, stream=None):
        """bdpt_sky_mis_execute: MIS sky lighting on the context's tile pixels — abi.SkyMisParams (frameCount, clampUpper,
        minT, samples, matIndex, techniques), the full-frame G-buffer, and the full-frame RGBA32F image at `out_ptr`, which
        gets (colour, 1).  matIndex 0 needs a camera."""
        self._check(self._lib.bdpt_sky_mis_execute(self._h, C.byref(params), C.byref(gbuffer), out_ptr, stream), "bdpt_sky_mis_execute")

    # ---- resampled direct lighting (include/bdpt.h "Resampled direct lighting") ----
    @staticmethod
    def _ris_mode(what, candidates, samples, mat_index, area_lights, use_hints, clamp):
        """(candidates, samples, matIndex, flags, clampUpper) of a resampled direct lighting call, checked."""
        for name, v, top in (("candidates", candidates, abi.RIS_MAX_CANDIDATES), ("samples", samples, abi.RIS_MAX_SAMPLES)):
            if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= top:
                raise BdptError(f"{what}: {name} must be an integer in 1 .. {top}, not {v!r}")
        mat, _ = Context._bsdf_mode(what, mat_index, False)
        for name, v in (("area_lights", area_lights), ("use_hints", use_hints)):
            if not isinstance(v, bool):
                raise BdptError(f"{what}: {name} must be a bool, not {v!r}")
        if isinstance(clamp, bool) or not isinstance(clamp, (int, float)) or not float(clamp) >= 0.0:
            raise BdptError(f"{what}: clamp must be a number >= 0, not {clamp!r}")
        flags = (abi.PARAM_AREA_LIGHTS if area_lights else 0) | (abi.RIS_USE_HINTS if use_hints else 0)
        return candidates, samples, mat, flags, float(clamp)

    def ris_lighting(self, surfaces, seeds, candidates, samples=1, mat_index=1, area_lights=False, use_hints=False,
                     clamp=float(3.4028234663852886e38), min_t=1e-4, alive=None, out=None, seeds_out=None, traced=None,
                     reservoirs=None, count=None, stream=None):
        """bdpt_ris_query: resampled direct lighting.  Per (N, 24) bdpt_surface record and sample, `candidates` (1 .. 32)
        next-event samples of the pass are drawn, one is kept with probability proportional to its unshadowed, clamped
        value at the record, and one any-hit ray is traced for it; `samples` (1 .. 64) such estimates are averaged — in one
        launch the loop sample_lights(seeds_out=) -> a draw -> clamp, weight and reservoir update, then trace_rays("any") ->
        ordered add, bit for bit.  seeds (N,) uint32 / int32 RNG states: two draws per candidate.  mat_index 0 GGX, 1
        Lambertian; area_lights makes the emitter table one more candidate source; use_hints tries a selected point or spot
        light's occluder hint before the ray (the same answer, fewer traversals); `clamp` bounds every component of a
        candidate's value.  Returns (N, 4) float32 (colour, 1); a miss record, or an item whose `alive` byte is 0, gives
        (diffuse, 1) without a draw.  GPU tensors only: alive (N,) uint8; seeds_out (N,) the states after the draws (it may
        be `seeds`); traced (N,) the rays traversed; reservoirs (N, samples, 4) int32 / uint32 in the bdpt_ris_reservoir
        layout (light | status << 16, the selected state, W and wsum as float bits).  `out` and `count` as for the other
        queries."""
        import torch
        records, words = (torch.float32, torch.int32), (torch.int32, torch.uint32)
        candidates, samples, mat, flags, clamp = self._ris_mode("ris_lighting", candidates, samples, mat_index, area_lights,
                                                                use_hints, clamp)
        extras = [("alive", alive, None, (torch.uint8,)), ("seeds_out", seeds_out, None, words), ("traced", traced, None, words)]
        if reservoirs is not None:
            n = int(surfaces.shape[0]) if getattr(surfaces, "is_cuda", False) and surfaces.dim() >= 1 else -1
            if n < 0:
                raise BdptError("ris_lighting: reservoirs goes with GPU tensor inputs")
            self._check_gpu(reservoirs, "ris_lighting", "reservoirs", (n, samples, 4), words)

        def run(ptrs, n, cnt, res):
            d = abi.RisDesc()
            d.num, d.flags, d.numDevice, d.matIndex, d.candidates, d.samples = n, flags, cnt, mat, candidates, samples
            d.clampUpper, d.minT = clamp, float(min_t)
            d.surfaces, d.seeds, d.color = ptrs[0], ptrs[1], res
            d.alive, d.seedsOut, d.traced, d.reservoirs = (None if t is None else t.data_ptr()
                                                           for t in (alive, seeds_out, traced, reservoirs))
            return self._lib.bdpt_ris_query(self._h, C.byref(d), stream)

        return self._surface_query("ris_lighting", [("surfaces", surfaces, 24, records), ("seeds", seeds, None, words)],
                                   (4, (torch.float32,)), run, out, count, extras=extras, fn="bdpt_ris_query")

    def ris_execute(self, gbuffer, out, *, candidates, samples=1, mat_index=1, area_lights=False, use_hints=False,
                    clamp=float(3.4028234663852886e38), min_t=1e-4, frame_count=0, reservoirs=None, stream=None):
        """bdpt_ris_execute: resampled direct lighting on the context's tile pixels — the full-frame G-buffer (abi.GBuffer)
        and the full-frame (H, W, 4) float32 GPU image `out`, which gets (colour, 1) at the tile's pixels; seeds are
        initRand(pixel, frame_count).  mat_index 0 needs a camera.  reservoirs (bdpt_ris_execute_reservoirs): a full-frame
        (H, W, samples, 4) int32 / uint32 GPU image that gets the bdpt_ris_reservoir records of the tile's geometry pixels.
        Returns the abi.RisParams used."""
        import torch
        candidates, samples, mat, flags, clamp = self._ris_mode("ris_execute", candidates, samples, mat_index, area_lights,
                                                                use_hints, clamp)
        if not isinstance(gbuffer, abi.GBuffer):
            raise BdptError("ris_execute: gbuffer must be an abi.GBuffer")
        frame = getattr(self, "_frame", None)
        if frame is None:
            raise BdptError("ris_execute: no frame size (resize first)")
        self._check_gpu(out, "ris_execute", "out", frame + (4,), (torch.float32,))
        p = abi.RisParams()
        p.frameCount, p.clampUpper, p.minT = int(frame_count) & 0xFFFFFFFF, clamp, float(min_t)
        p.candidates, p.samples, p.matIndex, p.flags = candidates, samples, mat, flags
        if reservoirs is not None:
            self._check_gpu(reservoirs, "ris_execute", "reservoirs", frame + (samples, 4), (torch.int32, torch.uint32))
            self._check(self._lib.bdpt_ris_execute_reservoirs(self._h, C.byref(p), C.byref(gbuffer), C.c_void_p(out.data_ptr()),
                                                              C.c_void_p(reservoirs.data_ptr()), stream), "bdpt_ris_execute_reservoirs")
            return p
        self._check(self._lib.bdpt_ris_execute(self._h, C.byref(p), C.byref(gbuffer), C.c_void_p(out.data_ptr()), stream),
                    "bdpt_ris_execute")
        return p

    def reuse_execute(self, gbuffer, out, reservoirs, *, neighbors=0, radius=0, same_pixel=False, neighbor_index=None, pool_gbuffer=None,
                      pool_reservoirs=None, pool_camera_pos=(0.0, 0.0, 0.0), in_m=0, pool_m=0, max_m=abi.REUSE_MAX_M,
                      normal_min=float("-inf"), plane_max=float("inf"), mat_index=1, area_lights=False,
                      clamp=float(3.4028234663852886e38), min_t=1e-4, frame_count=0, reservoirs_out=None, stream=None):
        """bdpt_reuse_execute: reservoir reuse on the context's tile pixels.  `reservoirs` (H, W, 4) int32 / uint32: the
        pixels' own records; the pool is pool_gbuffer (abi.GBuffer; None: `gbuffer`) with pool_reservoirs (None:
        `reservoirs`) and, for mat_index 0, pool_camera_pos.  Neighbours: neighbor_index (H, W, neighbors) of pool pixels, or
        same_pixel (neighbors 1: the temporal pass), or offsets drawn within `radius`.  `out` (H, W, 4) float32 gets
        (colour, 1) and reservoirs_out (H, W, 4) the combined records at the tile's pixels; seeds are
        initRand(initRand(pixel, frame_count), 0x52455553).  The other arguments as reuse_lighting.  Returns the
        abi.ReuseParams used."""
        import torch
        what = "reuse_execute"
        words = (torch.int32, torch.uint32)
        _, _, mat, flags, clamp = self._ris_mode(what, 1, 1, mat_index, area_lights, False, clamp)
        for name, v, top in (("neighbors", neighbors, abi.REUSE_MAX_NEIGHBORS), ("radius", radius, abi.REUSE_MAX_RADIUS),
                             ("in_m", in_m, 2**32 - 1), ("pool_m", pool_m, 2**32 - 1), ("max_m", max_m, 2**32 - 1)):
            if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= top:
                raise BdptError(f"{what}: {name} must be an integer in 0 .. {top}, not {v!r}")
        if not isinstance(same_pixel, bool):
            raise BdptError(f"{what}: same_pixel must be a bool, not {same_pixel!r}")
        if same_pixel and (neighbor_index is not None or neighbors != 1):
            raise BdptError(f"{what}: same_pixel goes with neighbors=1 and no neighbor_index")
        if neighbors and not same_pixel and neighbor_index is None and radius < 1:
            raise BdptError(f"{what}: drawn offsets need a radius in 1 .. {abi.REUSE_MAX_RADIUS}")
        for name, g in (("gbuffer", gbuffer), ("pool_gbuffer", gbuffer if pool_gbuffer is None else pool_gbuffer)):
            if not isinstance(g, abi.GBuffer):
                raise BdptError(f"{what}: {name} must be an abi.GBuffer")
        frame = getattr(self, "_frame", None)
        if frame is None:
            raise BdptError(f"{what}: no frame size (resize first)")
        self._check_gpu(out, what, "out", frame + (4,), (torch.float32,))
        self._check_gpu(reservoirs, what, "reservoirs", frame + (4,), words)
        pool_reservoirs = reservoirs if pool_reservoirs is None else pool_reservoirs
        self._check_gpu(pool_reservoirs, what, "pool_reservoirs", frame + (4,), words)
        if neighbor_index is not None:
            self._check_gpu(neighbor_index, what, "neighbor_index", frame + (neighbors,), words)
        if reservoirs_out is not None:
            self._check_gpu(reservoirs_out, what, "reservoirs_out", frame + (4,), words)
            if reservoirs_out.data_ptr() in (reservoirs.data_ptr(), pool_reservoirs.data_ptr()):
                raise BdptError(f"{what}: reservoirs_out must be neither reservoirs nor pool_reservoirs")
        p = abi.ReuseParams()
        p.frameCount, p.clampUpper, p.minT, p.matIndex = int(frame_count) & 0xFFFFFFFF, clamp, float(min_t), mat
        p.flags, p.neighbors, p.radius = flags | (abi.REUSE_SAME_PIXEL if same_pixel else 0), neighbors, radius
        p.inM, p.poolM, p.maxM, p.normalMin, p.planeMax = in_m, pool_m, max_m, float(normal_min), float(plane_max)
        p.poolCameraPos = (C.c_float * 3)(*[float(v) for v in pool_camera_pos])
        setattr(p, "in", reservoirs.data_ptr())
        pool_gb = gbuffer if pool_gbuffer is None else pool_gbuffer
        p.poolGbuffer, p.pool = C.pointer(pool_gb), pool_reservoirs.data_ptr()
        p.neighborIndex = None if neighbor_index is None else neighbor_index.data_ptr()
        p.outReservoirs = None if reservoirs_out is None else reservoirs_out.data_ptr()
        self._check(self._lib.bdpt_reuse_execute(self._h, C.byref(p), C.byref(gbuffer), C.c_void_p(out.data_ptr()), stream),
                    "bdpt_reuse_execute")
        return p

    # ---- reservoir reuse (include/bdpt.h "Reservoir reuse") ----
    def reuse_lighting(self, surfaces, seeds, reservoirs, neighbor_index=None, pool_surfaces=None, pool_reservoirs=None,
                       pool_alive=None, in_m=0, pool_m=0, max_m=abi.REUSE_MAX_M, normal_min=float("-inf"), plane_max=float("inf"),
                       mat_index=1, area_lights=False, clamp=float(3.4028234663852886e38), min_t=1e-4, alive=None, out=None,
                       seeds_out=None, traced=None, reservoirs_out=None, count=None, stream=None):
        """bdpt_reuse_query: reservoir reuse, the second stage of ReSTIR.  Per (N, 24) bdpt_surface record its own reservoir
        (`reservoirs`, (N, 4) int32 / uint32 words: light | status << 16, state, W as float bits, M) and those of the pool
        entries `neighbor_index` (N, neighbors) names (neighbors 0 .. 8; an index >= the pool's length, such as -1, is no
        neighbour) are combined by the unbiased 1 / Z rule and one any-hit ray is traced for the survivor — in one launch
        the loop prev(state) -> sample_lights -> clamp, weight and reservoir update per source, the selected sample again
        at every neighbour for Z, then trace_rays("any"), bit for bit.  seeds (N,) RNG states: 1 + neighbors draws.  The
        pool is pool_surfaces (P, 24), pool_reservoirs (P, 4) and the optional pool_alive (P,) uint8, or, when
        pool_surfaces is None, the items themselves.  in_m / pool_m: non-zero, the candidate count of every own / pool
        record (bdpt_ris_query's records: its `candidates`), 0: the records' fourth word; max_m caps a pool record's
        count.  A neighbour needs dot(N, N_p) >= normal_min and |dot(N, pos_p - pos)| <= plane_max.  Returns (N, 4)
        float32 (colour, 1).  GPU tensors only: alive, seeds_out, traced (N,), reservoirs_out (N, 4), which must be neither
        `reservoirs` nor pool_reservoirs, neighbor_index and the pool.  `out` and `count` as for the other queries."""
        import torch
        what = "reuse_lighting"
        records, words = (torch.float32, torch.int32), (torch.int32, torch.uint32)
        _, _, mat, flags, clamp = self._ris_mode(what, 1, 1, mat_index, area_lights, False, clamp)
        for name, v in (("in_m", in_m), ("pool_m", pool_m), ("max_m", max_m)):
            if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 2**32:
                raise BdptError(f"{what}: {name} must be an integer in 0 .. 2^32 - 1, not {v!r}")
        for name, v in (("normal_min", normal_min), ("plane_max", plane_max)):
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise BdptError(f"{what}: {name} must be a number, not {v!r}")
        gpu_in = getattr(surfaces, "is_cuda", False) and surfaces.dim() >= 1
        n = int(surfaces.shape[0]) if gpu_in else -1
        own_pool = pool_surfaces is None
        if own_pool and (pool_reservoirs is not None or pool_alive is not None):
            raise BdptError(f"{what}: pool_reservoirs and pool_alive go with pool_surfaces")
        if any(t is not None for t in (neighbor_index, pool_surfaces, reservoirs_out)) and not gpu_in:
            raise BdptError(f"{what}: neighbor_index, the pool and reservoirs_out go with GPU tensor inputs")
        neighbors, pool_num = 0, 0
        if neighbor_index is not None:
            neighbors = int(neighbor_index.shape[1]) if getattr(neighbor_index, "is_cuda", False) and neighbor_index.dim() == 2 else -1
            if not 0 <= neighbors <= abi.REUSE_MAX_NEIGHBORS:
                raise BdptError(f"{what}: neighbor_index must be a GPU tensor (N, 0 .. {abi.REUSE_MAX_NEIGHBORS})")
            self._check_gpu(neighbor_index, what, "neighbor_index", (n, neighbors), words)
            if own_pool:
                pool_surfaces, pool_reservoirs, pool_alive, pool_num = surfaces, reservoirs, alive, n
            else:
                pool_num = int(pool_surfaces.shape[0]) if getattr(pool_surfaces, "is_cuda", False) and pool_surfaces.dim() >= 1 else -1
                if not 0 <= pool_num < 2**32:
                    raise BdptError(f"{what}: pool_surfaces must be a GPU tensor (P, 24)")
                self._check_gpu(pool_surfaces, what, "pool_surfaces", (pool_num, 24), records)
                if pool_reservoirs is None:
                    raise BdptError(f"{what}: pool_surfaces goes with pool_reservoirs")
                self._check_gpu(pool_reservoirs, what, "pool_reservoirs", (pool_num, 4), words)
                if pool_alive is not None:
                    self._check_gpu(pool_alive, what, "pool_alive", (pool_num,), (torch.uint8,))
        elif not own_pool:
            raise BdptError(f"{what}: a pool goes with neighbor_index")
        if reservoirs_out is not None:
            self._check_gpu(reservoirs_out, what, "reservoirs_out", (n, 4), words)
            for name, t in (("reservoirs", reservoirs), ("pool_reservoirs", pool_reservoirs if neighbors else None)):
                if n and getattr(t, "is_cuda", False) and t.data_ptr() == reservoirs_out.data_ptr():
                    raise BdptError(f"{what}: reservoirs_out must not be {name}")
        extras = [("alive", alive, None, (torch.uint8,)), ("seeds_out", seeds_out, None, words), ("traced", traced, None, words)]

        def run(ptrs, n, cnt, res):
            d = abi.ReuseDesc()
            d.num, d.flags, d.numDevice, d.matIndex, d.neighbors = n, flags, cnt, mat, neighbors
            d.inM, d.poolM, d.maxM, d.poolNum = in_m, pool_m, max_m, pool_num
            d.normalMin, d.planeMax, d.clampUpper, d.minT = float(normal_min), float(plane_max), clamp, float(min_t)
            d.surfaces, d.seeds, d.color = ptrs[0], ptrs[1], res
            setattr(d, "in", ptrs[2])
            d.alive, d.seedsOut, d.traced, d.out = (None if t is None else t.data_ptr() for t in (alive, seeds_out, traced, reservoirs_out))
            if neighbors:
                d.poolSurfaces, d.pool, d.neighborIndex = pool_surfaces.data_ptr(), pool_reservoirs.data_ptr(), neighbor_index.data_ptr()
                d.poolAlive = None if pool_alive is None else pool_alive.data_ptr()
            return self._lib.bdpt_reuse_query(self._h, C.byref(d), stream)

        return self._surface_query(what, [("surfaces", surfaces, 24, records), ("seeds", seeds, None, words),
                                          ("reservoirs", reservoirs, 4, words)],
                                   (4, (torch.float32,)), run, out, count, extras=extras, fn="bdpt_reuse_query")

    # ---- diffuse GI (include/bdpt.h "Diffuse GI") ----
    def diffuse_gi(self, surfaces, seeds, indirect=True, cosine=True, view_pos=None, normal_map=True, min_t=1e-4, alive=None,
                   out=None, hits=None, status=None, seeds_out=None, count=None, stream=None):
        """bdpt_gi_query: the reference's one-bounce path tracer per (N, 24) bdpt_surface record (posW, N, diffuse and prim
        are read), in one launch — the loop light_query -> trace_rays("any") -> sample_bsdf(mat_index=1) ->
        trace_rays("closest") -> shade_hits -> light_query -> trace_rays("any") and the shader's arithmetic, bit for bit.
        seeds (N,) uint32 / int32 RNG states: one draw, with `indirect` three.  cosine=False samples the hemisphere
        uniformly.  view_pos (three floats): the bounce hit is shaded as seen from there (the reference's behaviour, with
        the camera position), None: from the item's posW; normal_map as shade_hits'.  Returns (N, 4) float32 (colour, 1);
        a miss record (prim < 0), or an item whose `alive` byte is 0, gives (diffuse, 1) without a draw.  GPU tensors
        only: alive (N,) uint8; hits (N, 4) the bounce ray's hit; status (N,) abi.GI_STATUS_* bits; seeds_out (N,) the
        states after the draws (it may be `seeds`).  `out` and `count` as for the other queries."""
        import torch
        records, words = (torch.float32, torch.int32), (torch.int32, torch.uint32)  # the dtypes a record / a 32-bit word may have
        extras = [("alive", alive, None, (torch.uint8,)), ("hits", hits, 4, records), ("status", status, None, words),
                  ("seeds_out", seeds_out, None, words)]
        if view_pos is not None and len(view_pos) != 3:
            raise BdptError("diffuse_gi: view_pos must be three floats or None")

        def run(ptrs, n, cnt, res):
            d = abi.GiDesc()
            d.num, d.numDevice, d.minT = n, cnt, float(min_t)
            d.flags = (abi.GI_INDIRECT if indirect else 0) | (0 if cosine else abi.GI_UNIFORM) | \
                (abi.GI_SHADE_FROM_VIEW if view_pos is not None else 0)
            d.shadeFlags = abi.SHADE_NORMAL_MAP if normal_map else 0
            for k in range(3):
                d.viewPos[k] = float(view_pos[k]) if view_pos is not None else 0.0
            d.surfaces, d.seeds, d.color = ptrs[0], ptrs[1], res
            d.alive, d.hits, d.status, d.seedsOut = (None if t is None else t.data_ptr() for t in (alive, hits, status, seeds_out))
            return self._lib.bdpt_gi_query(self._h, C.byref(d), stream)

        return self._surface_query("diffuse_gi", [("surfaces", surfaces, 24, records), ("seeds", seeds, None, words)],
                                   (4, (torch.float32,)), run, out, count, extras=extras, fn="bdpt_gi_query")

    def gi_execute(self, params, gbuffer, out_ptr, stream=None):
        """bdpt_gi_execute: the reference's SimpleDiffuseGIPass on the context's tile pixels — abi.GiParams (frameCount, minT,
        flags), the full-frame G-buffer, and the full-frame RGBA32F image at `out_ptr`, which gets (colour, 1)."""
        self._check(self._lib.bdpt_gi_execute(self._h, C.byref(params), C.byref(gbuffer), out_ptr, stream), "bdpt_gi_execute")

    # ---- direct lighting (include/bdpt.h "Direct lighting") ----
    def direct_lighting(self, surfaces, *, alive=None, min_t, use_hints=False, visible=False, traced=False, out=None, count=None,
                        stream=None):
        """bdpt_direct_query: the reference's Lambertian-plus-shadows pass per (N, 24) bdpt_surface record (posW, N, diffuse,
        specular and prim are read): every light of the scene, at most one any-hit ray each, in one launch — the loop, per
        light, set_lights([light]) -> sample_lights(mat_index=1) -> trace_rays("any") -> accumulate, bit for bit.  No seeds:
        nothing is drawn.  use_hints tries the lights' occluder hints first (the same answer, fewer traversals).  Returns
        (N, 4) float32 (colour, 1); a miss record (prim < 0), or an item whose `alive` byte is 0, gives (diffuse, or specular
        where diffuse is black, 1).  visible / traced: False (not wanted), True (allocated) or an (N,) int32 / uint32 GPU
        tensor: per item bit k = light k was added unshadowed / a ray or hint test was spent on light k; with either the
        result is a tuple (colour, visible if wanted, traced if wanted).  GPU tensors only for alive, visible and traced.
        `out` and `count` as for the other queries."""
        import torch
        records, words = (torch.float32, torch.int32), (torch.int32, torch.uint32)  # the dtypes a record / a 32-bit word may have
        masks = []
        for name, m in (("visible", visible), ("traced", traced)):
            if m is True:
                if not getattr(surfaces, "is_cuda", False) or surfaces.dim() < 1:
                    raise BdptError(f"direct_lighting: {name}=True goes with GPU tensor inputs")
                m = torch.empty((int(surfaces.shape[0]),), dtype=torch.int32, device=surfaces.device)
            elif m is False:
                m = None
            elif m is None or isinstance(m, (bool, int, float)):
                raise BdptError(f"direct_lighting: {name} must be False, True or a GPU tensor, not {m!r}")
            masks.append(m)
        extras = [("alive", alive, None, (torch.uint8,)), ("visible", masks[0], None, words), ("traced", masks[1], None, words)]

        def run(ptrs, n, cnt, res):
            d = abi.DirectDesc()
            d.num, d.numDevice, d.minT, d.flags = n, cnt, float(min_t), abi.DIRECT_USE_HINTS if use_hints else 0
            d.surfaces, d.color = ptrs[0], res
            d.alive, d.visible, d.traced = (None if t is None else t.data_ptr() for t in (alive, masks[0], masks[1]))
            return self._lib.bdpt_direct_query(self._h, C.byref(d), stream)

        color = self._surface_query("direct_lighting", [("surfaces", surfaces, 24, records)], (4, (torch.float32,)), run, out, count,
                                    extras=extras, fn="bdpt_direct_query")
        wanted = [m for m in masks if m is not None]
        return (color, *wanted) if wanted else color

    def direct_execute(self, gbuffer, out, *, min_t, use_hints=False, stream=None):
        """bdpt_direct_execute: the reference's LambertianPlusShadowPass on the context's tile pixels — the full-frame G-buffer
        (abi.GBuffer) and the full-frame (H, W, 4) float32 GPU image `out`, which gets (colour, 1) at the tile's pixels."""
        import torch
        if not isinstance(gbuffer, abi.GBuffer):
            raise BdptError("direct_execute: gbuffer must be an abi.GBuffer")
        frame = getattr(self, "_frame", None)
        if frame is None:
            raise BdptError("direct_execute: no frame size (resize first)")
        self._check_gpu(out, "direct_execute", "out", frame + (4,), (torch.float32,))
        p = abi.DirectParams()
        p.minT, p.flags = float(min_t), abi.DIRECT_USE_HINTS if use_hints else 0
        self._check(self._lib.bdpt_direct_execute(self._h, C.byref(p), C.byref(gbuffer), C.c_void_p(out.data_ptr()), stream),
                    "bdpt_direct_execute")
        return p

    @staticmethod
    def _bsdf_mode(what, mat_index, from_lobe):
        if mat_index not in (0, 1) or isinstance(mat_index, bool):
            raise BdptError(f"{what}: mat_index must be 0 (GGX) or 1 (Lambertian), not {mat_index!r}")
        return int(mat_index), abi.PARAM_SPECULAR_FROM_LOBE if from_lobe else 0

    def _check_gpu(self, t, what, name, shape, dtypes):
        if not getattr(t, "is_cuda", False) or t.device.index != self.device:
            raise BdptError(f"{what}: {name} must be a GPU tensor on cuda:{self.device}, not on {getattr(t, 'device', type(t))}")
        if not t.is_contiguous():
            raise BdptError(f"{what}: {name} must be contiguous")
        if t.dtype not in dtypes or tuple(t.shape) != tuple(shape):
            raise BdptError(f"{what}: {name} must be {tuple(shape)} {'/'.join(str(d) for d in dtypes)}, not "
                            f"{tuple(t.shape)} {t.dtype}")

    def _surface_query(self, what, inputs, out_spec, run, out, count, extras=(), fn=None, any_count_shape=False):
        """The shared path of the per-item queries.  inputs: (name, value, columns or None for 1-D, allowed torch dtypes),
        all with one row per item; out_spec: (columns or None for 1-D, allowed dtypes; the first is allocated).  extras:
        further outputs of the same form that may be None and go with GPU tensor inputs only (a column count of 1 with a 1-D
        name "... count": a one-element tensor); fn: the library call's name for error messages; any_count_shape: `count`
        may be a one-element tensor of any shape (trace_rays), not only (1,)."""
        import numpy as np
        import torch
        on_gpu = [getattr(v, "is_cuda", False) for _, v, _, _ in inputs]
        if all(on_gpu):
            n = int(inputs[0][1].shape[0]) if inputs[0][1].dim() >= 1 else -1
            if n < 0 or n >= 2**32:
                raise BdptError(f"{what}: bad item count")
            for name, v, cols, dts in inputs:
                self._check_gpu(v, what, name, (n,) if cols is None else (n, cols), dts)
            if count is not None:
                one = any_count_shape and getattr(count, "is_cuda", False) and count.numel() == 1
                self._check_gpu(count, what, "count", tuple(count.shape) if one else (1,), (torch.int32, torch.uint32))
            for name, v, cols, dts in extras:
                if v is not None:
                    self._check_gpu(v, what, name, (1,) if name.endswith("count") else (n,) if cols is None else (n, cols), dts)
            out_shape = (n,) if out_spec[0] is None else (n, out_spec[0])
            if out is None:
                out = torch.empty(out_shape, dtype=out_spec[1][0], device=inputs[0][1].device)
            else:
                self._check_gpu(out, what, "out", out_shape, out_spec[1])
            self._check(run([v.data_ptr() for _, v, _, _ in inputs], n, None if count is None else count.data_ptr(), out.data_ptr()),
                        fn or "bdpt_" + ("bsdf_query" if "bsdf" in what else what))
            return out.view(torch.float32) if out.dtype == torch.int32 else out
        if any(on_gpu):
            raise BdptError(f"{what}: the inputs must all be GPU tensors or all host arrays")
        if out is not None or count is not None or any(v is not None for _, v, _, _ in extras):
            raise BdptError(f"{what}: out=, count= and the other output tensors go with GPU tensor inputs")
        np_of = {torch.float32: np.float32, torch.int32: np.int32, torch.uint32: np.uint32}
        host = []
        for name, v, cols, dts in inputs:
            if hasattr(v, "is_cuda") and getattr(v, "device", None) is not None and v.device.type != "cpu":
                raise BdptError(f"{what}: {name} on {v.device}: neither a GPU tensor nor host memory")
            a = v.detach().numpy() if hasattr(v, "detach") else v
            ok_types = {np.dtype(np_of[d]) for d in dts}
            if not isinstance(a, np.ndarray) or a.dtype not in ok_types or a.shape[1:] != (() if cols is None else (cols,)) \
                    or a.ndim != (1 if cols is None else 2):
                raise BdptError(f"{what}: {name} must be {'(N,)' if cols is None else f'(N, {cols})'} "
                                f"{'/'.join(str(np.dtype(np_of[d])) for d in dts)}")
            host.append(np.ascontiguousarray(a))
        if len({a.shape[0] for a in host}) != 1:
            raise BdptError(f"{what}: the inputs differ in length")
        if not torch.cuda.is_available():
            raise BdptError(f"{what}: no GPU visible to torch (the queries have no CPU fallback)")
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            devs = [_host_to_device(a, dev) for a in host]
            torch.cuda.synchronize(dev)  # the copies are done before the library's stream reads them
            res = self._surface_query(what, [(nm, d, c, t) for (nm, _, c, t), d in zip(inputs, devs)], out_spec, run, None, None,
                                      fn=fn)
            torch.cuda.synchronize(dev)
        return res.cpu().numpy()

    def set_lights(self, lights, stream=None):
        """bdpt_set_lights: the scene's lights moved (a sequence of abi.Light, as many as the scene has)."""
        arr = (abi.Light * len(lights))(*lights)
        self._check(self._lib.bdpt_set_lights(self._h, arr, len(lights), stream), "bdpt_set_lights")

    def refit_info(self):
        info = abi.RefitInfo()
        self._check(self._lib.bdpt_get_refit_info(self._h, C.byref(info)), "bdpt_get_refit_info")
        return info

    def recs_hash(self):
        """Test hook: FNV-1a over the context's acceleration-structure records as they stand (synchronises)."""
        h = C.c_uint64()
        self._check(self._lib.bdpt_ctx_recs_hash(self._h, C.byref(h)), "bdpt_ctx_recs_hash")
        return h.value

    def set_environment(self, env_map_ptr=None, width=0, height=0, color=(0.0, 0.0, 0.0, 0.0)):
        """What BDPT_PARAM_ENV_ON_MISS looks up: a device RGBA32F lat-long map, or a constant colour."""
        e = abi.Environment()
        e.envMap = env_map_ptr
        e.width, e.height = int(width), int(height)
        for i in range(4):
            e.color[i] = float(color[i])
        self._check(self._lib.bdpt_set_environment(self._h, C.byref(e)), "bdpt_set_environment")
        self._env_serial += 1  # (the library dropped the sampling table: env_prepare again)

    def resize(self, width, height, y0, y1, max_depth):
        self._check(self._lib.bdpt_resize(self._h, width, height, Tile(y0, y1), max_depth), "bdpt_resize")
        self._frame = (int(height), int(width))

    def resize_stripes(self, width, height, stripe_rows, num_owners, owner, max_depth):
        self._check(self._lib.bdpt_resize_stripes(self._h, width, height, Stripes(stripe_rows, num_owners, owner), max_depth),
                    "bdpt_resize_stripes")
        self._frame = (int(height), int(width))

    def tile_info(self):
        info = TileInfo()
        self._check(self._lib.bdpt_get_tile_info(self._h, C.byref(info)), "bdpt_get_tile_info")
        return info

    def row_ranges(self):
        n = self.tile_info().numRowRanges
        buf = (C.c_uint32 * (2 * max(n, 1)))()
        got = self._check(self._lib.bdpt_tile_row_ranges(self._h, buf, n), "bdpt_tile_row_ranges")
        return [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(got)]

    def resolve_tile(self, tile_splat_ptr, out_ptr, stream=None):
        self._check(self._lib.bdpt_resolve_tile(self._h, tile_splat_ptr, out_ptr, stream), "bdpt_resolve_tile")

    def accumulate_tile(self, last_ptr, cur_ptr, accum_count, max_count, stream=None):
        self._check(self._lib.bdpt_accumulate_tile(self._h, last_ptr, cur_ptr, accum_count, max_count, stream),
                    "bdpt_accumulate_tile")

    def gbuffer_execute(self, gparams, gbuffer, stream=None):
        self._check(self._lib.bdpt_gbuffer_execute(self._h, C.byref(gparams), C.byref(gbuffer), stream),
                    "bdpt_gbuffer_execute")

    def gbuffer_execute_motion(self, gparams, gbuffer, prev_position_ptr, stream=None):
        """bdpt_gbuffer_execute plus the PrevWorldPosition channel (W x H float4 at `prev_position_ptr`): where each pixel's
        surface point was in the previous pose (after prepare(motion=True))."""
        self._check(self._lib.bdpt_gbuffer_execute_motion(self._h, C.byref(gparams), C.byref(gbuffer), prev_position_ptr, stream),
                    "bdpt_gbuffer_execute_motion")

    def execute(self, params, gbuffer, out_ptr, stream=None):
        self._check(self._lib.bdpt_execute(self._h, C.byref(params), C.byref(gbuffer), out_ptr, stream), "bdpt_execute")

    def execute_light_groups(self, params, gbuffer, out_ptr, groups_ptr, stream=None):
        """bdpt_execute_light_groups: bdpt_execute into `out_ptr` plus (numLights + 1) RGBA32F planes of the frame at
        `groups_ptr` (plane k = light k, the last = emission; contract in include/bdpt.h "Light groups")."""
        self._check(self._lib.bdpt_execute_light_groups(self._h, C.byref(params), C.byref(gbuffer), out_ptr, groups_ptr, stream),
                    "bdpt_execute_light_groups")

    def execute_grouped(self, params, gbuffer, out_ptr, groups_ptr, assignment, num_groups, stream=None):
        """bdpt_execute_grouped: bdpt_execute into `out_ptr` plus (num_groups + 1) RGBA32F planes of the frame at
        `groups_ptr` (plane g = the lights `assignment` puts in group g, the last = emission).  `assignment` is a sequence
        of group indices, one per light, and with PARAM_AREA_LIGHTS one more for the emitter table; the library copies it
        before it returns (contract in include/bdpt.h "Assignable light groups")."""
        a = [int(g) for g in assignment]
        if any(g < 0 or g > 255 for g in a):
            raise BdptError(f"execute_grouped: group indices must be 0 .. 255, not {a!r}")
        arr = (C.c_uint8 * max(len(a), 1))(*a)
        d = abi.LightGroupDesc()
        d.planes = groups_ptr if isinstance(groups_ptr, (int, type(None))) else groups_ptr.value
        d.numGroups = int(num_groups)
        d.numAssigned = len(a)
        d.groupOf = C.cast(arr, C.POINTER(C.c_uint8))
        self._check(self._lib.bdpt_execute_grouped(self._h, C.byref(params), C.byref(gbuffer), out_ptr, C.byref(d), stream),
                    "bdpt_execute_grouped")

    def execute_masked(self, params, gbuffer, mask_ptr, out_ptr, stream=None):
        """bdpt_execute_masked: bdpt_execute for the pixels whose byte of `mask_ptr` (W x H uint8, device) is non-zero;
        the others' `out` is left as it is (contract in include/bdpt.h)."""
        self._check(self._lib.bdpt_execute_masked(self._h, C.byref(params), C.byref(gbuffer), mask_ptr, out_ptr, stream),
                    "bdpt_execute_masked")

    def adaptive_reset(self, state, stream=None):
        """bdpt_adaptive_reset: `state` is an abi.AdaptiveState of device pointers (mean = m2 = count = 0, mask = 1)."""
        self._check(self._lib.bdpt_adaptive_reset(self._h, C.byref(state), stream), "bdpt_adaptive_reset")

    def adaptive_update(self, params, state, frame_ptr, stream=None):
        """bdpt_adaptive_update: fold the frame at `frame_ptr` into `state`, write the next mask and the mean back to the
        frame.  `params` is an abi.AdaptiveParams or a dict for adaptive_params()."""
        if not isinstance(params, abi.AdaptiveParams):
            params = adaptive_params(params)
        self._check(self._lib.bdpt_adaptive_update(self._h, C.byref(params), C.byref(state), frame_ptr, stream),
                    "bdpt_adaptive_update")

    def execute_tail(self, params, gbuffer, out_ptr, stream=None):
        self._check(self._lib.bdpt_execute_tail(self._h, C.byref(params), C.byref(gbuffer), out_ptr, stream),
                    "bdpt_execute_tail")

    def prepare(self, what=0, motion=False, refit_pieces=False):
        """bdpt_prepare(what); motion=True adds PREPARE_MOTION (the previous pose of keep_pose; needs a scene),
        refit_pieces=True adds PREPARE_REFIT_PIECES (later updates refit split / clipped references by their piece; needs
        a scene that has not been updated yet)."""
        what = int(what) | (abi.PREPARE_MOTION if motion else 0) | (abi.PREPARE_REFIT_PIECES if refit_pieces else 0)
        self._check(self._lib.bdpt_prepare(self._h, what), "bdpt_prepare")

    def splat_buffer(self):
        p = C.c_void_p()
        n = C.c_uint64()
        self._check(self._lib.bdpt_splat_buffer(self._h, C.byref(p), C.byref(n)), "bdpt_splat_buffer")
        return p.value, n.value

    def set_splat_buffer(self, ptr, num_u64):
        self._check(self._lib.bdpt_set_splat_buffer(self._h, ptr, num_u64), "bdpt_set_splat_buffer")

    def resolve(self, splat_ptr, splat_row0, out_ptr, stream=None):
        self._check(self._lib.bdpt_resolve(self._h, splat_ptr, splat_row0, out_ptr, stream), "bdpt_resolve")

    def accumulate(self, last_ptr, cur_ptr, accum_count, max_count, num_texels, stream=None):
        self._check(self._lib.bdpt_accumulate(self._h, last_ptr, cur_ptr, accum_count, max_count, num_texels, stream),
                    "bdpt_accumulate")

    def bmfr_execute(self, params, gbuffer, noisy_ptr, stream=None):
        self._check(self._lib.bdpt_bmfr_execute(self._h, C.byref(params), C.byref(gbuffer), noisy_ptr, stream),
                    "bdpt_bmfr_execute")

    def bmfr_execute_motion(self, params, gbuffer, prev_position_ptr, noisy_ptr, stream=None):
        """bdpt_bmfr_execute reprojecting through the PrevWorldPosition channel at `prev_position_ptr` (W x H float4)."""
        self._check(self._lib.bdpt_bmfr_execute_motion(self._h, C.byref(params), C.byref(gbuffer), prev_position_ptr, noisy_ptr,
                                                       stream), "bdpt_bmfr_execute_motion")

    def bmfr_reset(self):
        self._check(self._lib.bdpt_bmfr_reset(self._h), "bdpt_bmfr_reset")

    def bmfr_planes_prepare(self, n):
        """bdpt_bmfr_planes_prepare: allocate the plane history of bmfr_execute_planes for `n` planes and reset it."""
        self._check(self._lib.bdpt_bmfr_planes_prepare(self._h, int(n)), "bdpt_bmfr_planes_prepare")

    def bmfr_planes_reset(self):
        self._check(self._lib.bdpt_bmfr_planes_reset(self._h), "bdpt_bmfr_planes_reset")

    def bmfr_execute_planes(self, params, gbuffer, planes, prev_position=None, stream=None):
        """bdpt_bmfr_execute_planes: denoise the images of `planes` in place, each to the bits bmfr_execute would give it on
        a context of its own, with the geometry tests and the fit's factorisation done once (contract in include/bdpt.h
        "Denoised planes").  `planes`: a (P, H, W, 4) float32 GPU tensor or a sequence of (H, W, 4) float32 GPU tensors, all
        of one shape, P = 1 .. abi.BMFR_MAX_PLANES; list position k owns history slot k.  `prev_position`: an (H, W, 4)
        float32 GPU tensor, the channel of bmfr_execute_motion, or None."""
        import torch
        what = "bmfr_execute_planes"
        if getattr(planes, "is_cuda", False) and hasattr(planes, "dim"):
            if planes.dim() != 4 or planes.shape[3] != 4:
                raise BdptError(f"{what}: planes must be (P, H, W, 4) float32, not {tuple(planes.shape)} {planes.dtype}")
            self._check_gpu(planes, what, "planes", tuple(planes.shape), (torch.float32,))
            count, frame = int(planes.shape[0]), tuple(planes.shape[1:])
            stride = frame[0] * frame[1] * 16
            ptrs = [planes.data_ptr() + k * stride for k in range(count)]
        else:
            try:
                items = list(planes)
            except TypeError:
                raise BdptError(f"{what}: planes must be a (P, H, W, 4) GPU tensor or a sequence of (H, W, 4) GPU tensors") from None
            count = len(items)
            frame = tuple(getattr(items[0], "shape", ())) if items else ()
            if count and (len(frame) != 3 or frame[2] != 4):
                raise BdptError(f"{what}: planes[0] must be (H, W, 4) float32, not {frame}")
            for k, t in enumerate(items):
                self._check_gpu(t, what, f"planes[{k}]", frame, (torch.float32,))
            ptrs = [t.data_ptr() for t in items]
        if not 1 <= count <= abi.BMFR_MAX_PLANES:
            raise BdptError(f"{what}: 1 .. {abi.BMFR_MAX_PLANES} planes, not {count}")
        size = getattr(self, "_frame", None)  # (set by resize / resize_stripes)
        if size is not None and frame != size + (4,):
            raise BdptError(f"{what}: the planes must be whole frames, {size + (4,)}, not {frame}")
        if prev_position is not None:
            self._check_gpu(prev_position, what, "prev_position", frame, (torch.float32,))
        arr = (C.c_void_p * count)(*ptrs)
        d = abi.BmfrPlanesDesc()
        d.planes = C.cast(arr, C.POINTER(C.c_void_p))
        d.numPlanes = count
        d.prevPosition = None if prev_position is None else prev_position.data_ptr()
        self._check(self._lib.bdpt_bmfr_execute_planes(self._h, C.byref(params), C.byref(gbuffer), C.byref(d), stream),
                    "bdpt_bmfr_execute_planes")

    def counters(self):
        c = Counters()
        self._check(self._lib.bdpt_get_counters(self._h, C.byref(c)), "bdpt_get_counters")
        return c

    def enable_stage_timing(self, on=True):
        self._check(self._lib.bdpt_enable_stage_timing(self._h, 1 if on else 0), "bdpt_enable_stage_timing")

    def stage_times(self):
        names = (C.c_char_p * 64)()
        ms = (C.c_float * 64)()
        n = self._check(self._lib.bdpt_get_stage_times(self._h, names, ms, 64), "bdpt_get_stage_times")
        return [(names[i].decode(), float(ms[i])) for i in range(n)]

    def sync(self, stream=None):
        self._check(self._lib.bdpt_sync(self._h, stream), "bdpt_sync")

    # test hooks -------------------------------------------------------------------------------
    def test_rng(self, val0, val1, draws):
        import numpy as np
        val0 = np.ascontiguousarray(val0, np.uint32)
        val1 = np.ascontiguousarray(val1, np.uint32)
        n = val0.size
        st = np.zeros((n, draws), np.uint32)
        fl = np.zeros((n, draws), np.float32)
        self._check(self._lib.bdpt_test_rng(self._h, val0.ctypes.data, val1.ctypes.data, n, draws, st.ctypes.data,
                                            fl.ctypes.data), "bdpt_test_rng")
        return st, fl

    def test_trace(self, rays, mode):
        import numpy as np
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        n = rays.shape[0]
        prim = np.zeros(n, np.int32)
        tuv = np.zeros((n, 3), np.float32)
        self._check(self._lib.bdpt_test_trace(self._h, rays.ctypes.data, n, mode, prim.ctypes.data, tuv.ctypes.data),
                    "bdpt_test_trace")
        return prim, tuv

    def test_trace_shadow(self, rays):
        """The persistent any-hit kernel over host rays (n x 8 float32): visibility bytes and the deepest stack reached."""
        import numpy as np
        rays = np.ascontiguousarray(rays, np.float32)
        n = rays.shape[0]
        vis = np.zeros(n, np.uint8)
        deep = C.c_uint32(0)
        self._check(self._lib.bdpt_test_trace_shadow(self._h, rays.ctypes.data, n, vis.ctypes.data, C.byref(deep)),
                    "bdpt_test_trace_shadow")
        return vis, deep.value

    def test_bsdf(self, recs, mat_index):
        import numpy as np
        recs = np.ascontiguousarray(recs, np.float32).reshape(-1, 20)
        out = np.zeros((recs.shape[0], 16), np.float32)
        self._check(self._lib.bdpt_test_bsdf(self._h, recs.ctypes.data, recs.shape[0], mat_index, out.ctypes.data),
                    "bdpt_test_bsdf")
        return out

    def area_light_info(self):
        """bdpt_get_area_light_info: the emitter table of PARAM_AREA_LIGHTS (made if need be; synchronises)."""
        info = abi.AreaLightInfo()
        self._check(self._lib.bdpt_get_area_light_info(self._h, C.byref(info)), "bdpt_get_area_light_info")
        return info

    def test_area_light_sample(self, mode, states, points=None):
        """Test hook bdpt_test_area_light_sample: (n, 16) float32 records (include/bdpt.h lists the fields).
        states: RNG states right after the selection draw; points: (n, 3) receiving points for mode 1."""
        import numpy as np
        states = np.ascontiguousarray(states, np.uint32).reshape(-1)
        n = states.shape[0]
        pts = None
        if points is not None:
            pts = np.ascontiguousarray(points, np.float32).reshape(n, 3)
        out = np.zeros((n, 16), np.float32)
        self._check(self._lib.bdpt_test_area_light_sample(self._h, mode, states.ctypes.data,
                                                          None if pts is None else pts.ctypes.data, n, out.ctypes.data),
                    "bdpt_test_area_light_sample")
        return out

    def test_alpha(self, variant, prim, uv):
        """Test hook bdpt_test_alpha: the any-hit alpha verdict of each (prim, u, v) -> (n,) bool, True where the candidate is
        ignored.  variant 0: alphaTestFails; 1 and 2: the first and the second slot of alphaTestFails2 (include/bdpt.h)."""
        import numpy as np
        prim = np.ascontiguousarray(prim, np.uint32).reshape(-1)
        uv = np.ascontiguousarray(uv, np.float32).reshape(prim.shape[0], 2)
        out = np.zeros(prim.shape[0], np.uint8)
        self._check(self._lib.bdpt_test_alpha(self._h, variant, prim.ctypes.data, uv.ctypes.data, prim.shape[0], out.ctypes.data),
                    "bdpt_test_alpha")
        return out != 0

    def close(self):
        if self._h:
            self._lib.bdpt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# Defaults of FramePipeline(adaptive={...}): measured on the bench frame (profiles/README.md "Adaptive sampling").
ADAPTIVE_DEFAULTS = {"threshold": 0.15, "epsilon": 1e-3, "min_samples": 8, "max_samples": 256, "block_size": 8}


def adaptive_params(d=None):
    """abi.AdaptiveParams from a dict of ADAPTIVE_DEFAULTS' keys (missing keys take the defaults).  The checks are
    bdpt_adaptive_update's, made here too so that a bad setting fails before a GPU is touched."""
    d = dict(d or {})
    unknown = set(d) - set(ADAPTIVE_DEFAULTS)
    if unknown:
        raise BdptError(f"adaptive: unknown setting(s) {sorted(unknown)}; known: {sorted(ADAPTIVE_DEFAULTS)}")
    v = dict(ADAPTIVE_DEFAULTS, **d)
    b, lo, hi = int(v["block_size"]), int(v["min_samples"]), int(v["max_samples"])
    if b not in (1, 2, 4, 8, 16):
        raise BdptError(f"adaptive: block_size must be 1, 2, 4, 8 or 16, not {v['block_size']!r}")
    if lo < 2 or hi < lo:
        raise BdptError(f"adaptive: need 2 <= min_samples <= max_samples (got {lo}, {hi})")
    if hi >= 2 ** 32:
        raise BdptError("adaptive: max_samples must fit in 32 bits")
    return abi.AdaptiveParams(float(v["threshold"]), float(v["epsilon"]), lo, hi, b)


class FramePipeline:
    """The reference's per-frame sequence for this path on one GPU / one tile.

    Pass 0 LightProbeGBufferPass (frame counter starts 0xdeadbeef, CommonPasses/LightProbeGBufferPass.h:79),
    pass 1 BDPTPass (0x1337, BDPTPass.h:44), pass 2 SimpleAccumulationPass (cap 100 by default,
    CommonPasses/SimpleAccumulationPass.h:70).  Channels live in torch tensors on ``cuda:<device>``.

    light_groups=True renders every frame with bdpt_execute_light_groups: ``light_groups`` is a (numLights + 1, H, W, 4)
    float32 tensor with the frame's planes (plane k = light k, the last = emission) and ``light_groups_accum`` their
    running means, kept by one bdpt_accumulate over all planes with the beauty's counters.  As the beauty's ``output``,
    ``light_groups`` holds the mean too after an accumulating frame.  Whole frames only: not with a tile or stripes.
    light_groups=<sequence of group indices> (one per light; with flags=PARAM_AREA_LIGHTS one more, for the emitter
    table) renders through bdpt_execute_grouped instead: the tensors are of shape (max(assignment) + 2, H, W, 4), plane g
    the lights assigned to group g, the last emission.

    adaptive={...} (settings of ADAPTIVE_DEFAULTS; {} for the defaults) makes every frame adaptive: bdpt_execute_masked
    renders the pixels of ``adaptive_state["mask"]`` and bdpt_adaptive_update folds them into the per-pixel running mean
    (``adaptive_state``: mean, m2, count, mask, active), which ``output`` then shows.  This replaces the accumulation
    pass: render_frame's ``accumulate`` has no effect.  active_pixels() reads how many pixels the next frame renders (0:
    the image has converged); adaptive_reset() starts over (after a camera, scene or light change).  Whole frames only,
    and not with light_groups.

    motion=True keeps the previous pose (Context.prepare(motion=True)): every G-buffer pass also writes ``prev_position``
    ((H, W, 4) float32: where each pixel's surface point was at the previous frame's G-buffer pass, for
    Context.bmfr_execute_motion), and render_frame ends its G-buffer stage with keep_pose, so that the updates a caller
    issues between two render_frame calls are measured against the pose the earlier frame rendered, and a frame without
    an update gets zero motion.

    denoise_groups=<BMFR_* flags> (with light_groups) denoises the planes after every render_frame with one
    Context.bmfr_execute_planes: ``light_groups_denoised`` ((planes + 1, H, W, 4) float32) holds the denoised copies of the
    ``light_groups`` planes and, last, that of ``output``; the rendered tensors stay as they are.  Entry k is what
    bdpt_bmfr_execute gives that image on a context of its own.  The pipeline keeps the previous frame's view-projection
    (view_proj_of_camera of ``cam``) for prevViewProj, counts the denoiser's frames from 0 (``last_denoise_params``: the
    BmfrParams of the last frame; denoise_reset() starts over) and passes ``prev_position`` when motion=True.  Relighting
    is a torch expression over the tensor: ``(gains[:, None, None, None] * pipe.light_groups_denoised[:-1]).sum(0)``.
    """

    def __init__(self, scene, width, height, max_depth=3, mat_index=0, device=0, tile=None, clamp_upper=0.9, min_t=1e-4,
                 accum_limit=100, flags=0, stripes=None, light_groups=False, adaptive=None, motion=False, denoise_groups=None):
        import torch
        self.torch = torch
        if denoise_groups is not None and (light_groups is None or light_groups is False):
            raise BdptError("denoise_groups needs light_groups: it denoises the light-group planes")
        self.denoise_flags = None if denoise_groups is None else int(denoise_groups)
        self.adaptive_params = None if adaptive is None else adaptive_params(adaptive)
        if adaptive is not None and (light_groups or stripes is not None or
                                     (tile is not None and (int(tile[0]), int(tile[1])) != (0, int(height)))):
            raise BdptError("adaptive sampling needs a pipeline that renders the whole frame (no tile, no stripes) without "
                            "light groups")
        self.group_assignment = None
        if not isinstance(light_groups, bool) and light_groups is not None:
            self.group_assignment = [int(g) for g in light_groups]
            want = int(scene.desc.numLights) + (1 if int(flags) & abi.PARAM_AREA_LIGHTS else 0)
            if len(self.group_assignment) != want:
                raise BdptError(f"light groups: the assignment needs {want} entries (one per light, and one for the emitter "
                                f"table with PARAM_AREA_LIGHTS), not {len(self.group_assignment)}")
            if not self.group_assignment or min(self.group_assignment) < 0 or max(self.group_assignment) > abi.BDPT_MAX_LIGHTS:
                raise BdptError(f"light groups: group indices must be 0 .. {abi.BDPT_MAX_LIGHTS}, not {self.group_assignment!r}")
            light_groups = True
        if light_groups and (stripes is not None or (tile is not None and (int(tile[0]), int(tile[1])) != (0, int(height)))):
            raise BdptError("light groups need a pipeline that renders the whole frame (no tile, no stripes)")
        if not torch.cuda.is_available():
            raise BdptError("no GPU visible to torch: the render pass cannot run (no CPU fallback)")
        self.W, self.H = int(width), int(height)
        self.y0, self.y1 = (0, self.H) if tile is None else (int(tile[0]), int(tile[1]))
        self.max_depth, self.mat_index = int(max_depth), int(mat_index)
        self.clamp_upper, self.min_t, self.flags = float(clamp_upper), float(min_t), int(flags)
        self.accum_limit = int(accum_limit)
        self.dev = torch.device("cuda", device)
        import time
        t0 = time.time()
        self.ctx = Context(device)
        t1 = time.time()
        # The frame's buffers first, the scene second: building the acceleration structure of a large scene takes and
        # frees some 15 GB of device scratch, and the driver clears VRAM that has been used before when it hands it out
        # again (~35 GB/s) — a 94 GB bdpt_resize issued right after such a bdpt_set_scene was measured 1-1.7 s slower
        # (0.01-0.03 s on untouched memory).
        # tile = (y0, y1): a contiguous band; stripes = (stripe_rows, num_owners, owner): interleaved stripes
        self.stripes = stripes
        if stripes is None:
            self.ctx.resize(self.W, self.H, self.y0, self.y1, self.max_depth)
        else:
            self.ctx.resize_stripes(self.W, self.H, int(stripes[0]), int(stripes[1]), int(stripes[2]), self.max_depth)
        self.rows = self.ctx.row_ranges()
        torch.cuda.synchronize(self.dev)
        t2 = time.time()
        self.scene = scene
        self.ctx.set_scene(scene.desc)
        self.cam = scene.camera(self.W / self.H)
        self.ctx.set_camera(self.cam)
        t3 = time.time()
        with torch.cuda.device(self.dev):
            self.channels = {"WorldPosition": torch.zeros(self.H, self.W, 4, dtype=torch.float32, device=self.dev)}
            for name in GBUFFER_CHANNELS[1:]:
                self.channels[name] = torch.zeros(self.H, self.W, 4, dtype=torch.float16, device=self.dev)
            self.channels[OUTPUT_CHANNEL] = torch.zeros(self.H, self.W, 4, dtype=torch.float32, device=self.dev)
            self.last_frame = torch.zeros(self.H, self.W, 4, dtype=torch.float32, device=self.dev)
            self.light_groups = self.light_groups_accum = None
            if light_groups:
                k = int(scene.desc.numLights) + 1 if self.group_assignment is None else max(self.group_assignment) + 2
                self.light_groups = torch.zeros(k, self.H, self.W, 4, dtype=torch.float32, device=self.dev)
                self.light_groups_accum = torch.zeros(k, self.H, self.W, 4, dtype=torch.float32, device=self.dev)
            self.light_groups_denoised = None
            if self.denoise_flags is not None:
                self.light_groups_denoised = torch.zeros(k + 1, self.H, self.W, 4, dtype=torch.float32, device=self.dev)
                self.ctx.bmfr_planes_prepare(k + 1)
            self.prev_position = None
            if motion:
                self.ctx.prepare(motion=True)
                self.prev_position = torch.zeros(self.H, self.W, 4, dtype=torch.float32, device=self.dev)
            self.adaptive_state = None
            if adaptive is not None:
                self.adaptive_state = {
                    "mean": torch.zeros(self.H, self.W, 4, dtype=torch.float32, device=self.dev),
                    "m2": torch.zeros(self.H, self.W, dtype=torch.float32, device=self.dev),
                    "count": torch.zeros(self.H, self.W, dtype=torch.int32, device=self.dev),  # (uint32 in the library)
                    "mask": torch.ones(self.H, self.W, dtype=torch.uint8, device=self.dev),
                    "active": torch.zeros(1, dtype=torch.int32, device=self.dev),
                }
                st = self.adaptive_state
                self._adaptive_c = abi.AdaptiveState(*[st[k].data_ptr() for k in ("mean", "m2", "count", "mask", "active")])
                self.ctx.adaptive_reset(self._adaptive_c, C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream))
        torch.cuda.synchronize(self.dev)
        # where the set-up time went: the scene (acceleration structure + uploads) and the frame's buffers are separate things
        self.setup_times = {"context_s": t1 - t0, "resize_s": t2 - t1, "set_scene_s": t3 - t2, "channels_s": time.time() - t3}
        self.gb = GBuffer(*[self.channels[n].data_ptr() for n in GBUFFER_CHANNELS])
        self.gbuffer_frame = 0xdeadbeef
        self.bdpt_frame = 0x1337
        self.ao_frame = 0  # CommonPasses/AmbientOcclusionPass.h:54
        self.last_ao_params = None
        self._ao_radius = None  # the pass's default radius for the scene, made on first use
        self.last_direct_params = None
        self.sky_frame = 0
        self.last_sky_params = None
        self.ris_frame = 0
        self.last_ris_params = None
        self.restir_frame = 0
        self._restir = None  # restir_lighting's reservoir buffers and history, made on first use
        self.gi_frame = 0x1337  # CommonPasses/SimpleDiffuseGIPass.h:62
        self.last_gi_params = None
        self.accum_count = 0
        self.env_color = (0.5, 0.5, 0.8, 1.0)  # SharedUtils/ResourceManager.cpp:77-87 default environment
        self.use_jitter = True
        self.last_params = None
        self.denoise_frame = 0
        self.last_denoise_params = None
        self._prev_view_proj = None

    @property
    def output(self):
        return self.channels[OUTPUT_CHANNEL]

    def _stream_ptr(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def gbuffer_params(self):
        gp = GBufferParams()
        if self.use_jitter:
            gp.pixelJitter[0], gp.pixelJitter[1] = msaa_jitter(self.gbuffer_frame)
        else:
            gp.pixelJitter[0], gp.pixelJitter[1] = 0.5, 0.5
        gp.frameCount = self.gbuffer_frame & 0xFFFFFFFF
        gp.useThinLens = 0
        gp.focalLen = 1.0
        gp.lensRadius = 1.0 / 64.0  # mFocalLength / (2 mFStop), LightProbeGBufferPass.cpp:117
        gp.envMap = None
        gp.envWidth = gp.envHeight = 128
        for i in range(4):
            gp.envColor[i] = self.env_color[i]
        return gp

    def bdpt_params(self, extra_flags=0):
        p = Params()
        p.minT = self.min_t
        p.frameCount = self.bdpt_frame & 0xFFFFFFFF
        p.matIndex = self.mat_index
        p.refractiveIndex = 1.0
        p.maxDepth = self.max_depth
        p.emitMult = 1.0
        p.clampUpper = self.clamp_upper
        p.pixelJitter[0], p.pixelJitter[1] = msaa_jitter(self.bdpt_frame)
        p.flags = self.flags | extra_flags
        return p

    def render_frame(self, accumulate=False, extra_flags=0, gbuffer=True):
        """One pipeline frame.  Returns the bdpt_params used (for the oracle to mirror)."""
        st = self._stream_ptr()
        gp = self.gbuffer_params()
        if gbuffer and self.prev_position is not None:
            self.ctx.gbuffer_execute_motion(gp, self.gb, C.c_void_p(self.prev_position.data_ptr()), st)
            self.ctx.keep_pose(st)  # (the start of the next step: before the updates the caller issues for it)
        elif gbuffer:
            self.ctx.gbuffer_execute(gp, self.gb, st)
        p = self.bdpt_params(extra_flags)
        if self.adaptive_state is not None:
            self.ctx.execute_masked(p, self.gb, C.c_void_p(self.adaptive_state["mask"].data_ptr()), C.c_void_p(self.output.data_ptr()), st)
            self.ctx.adaptive_update(self.adaptive_params, self._adaptive_c, C.c_void_p(self.output.data_ptr()), st)
            self.gbuffer_frame += 1
            self.bdpt_frame += 1
            self.last_params = (gp, p)
            return gp, p
        if self.light_groups is None:
            self.ctx.execute(p, self.gb, C.c_void_p(self.output.data_ptr()), st)
        elif self.group_assignment is None:
            self.ctx.execute_light_groups(p, self.gb, C.c_void_p(self.output.data_ptr()), C.c_void_p(self.light_groups.data_ptr()), st)
        else:
            self.ctx.execute_grouped(p, self.gb, C.c_void_p(self.output.data_ptr()), C.c_void_p(self.light_groups.data_ptr()),
                                     self.group_assignment, self.light_groups.shape[0] - 1, st)
        self.gbuffer_frame += 1
        self.bdpt_frame += 1
        if accumulate:
            n = self.accum_count if self.accum_count < self.accum_limit else self.accum_limit
            if self.accum_count < self.accum_limit:
                self.accum_count += 1
            if self.stripes is None:
                self.ctx.accumulate(C.c_void_p(self.last_frame.data_ptr()), C.c_void_p(self.output.data_ptr()), n,
                                    self.accum_limit, self.W * self.H, st)
                if self.light_groups is not None:
                    self.ctx.accumulate(C.c_void_p(self.light_groups_accum.data_ptr()), C.c_void_p(self.light_groups.data_ptr()), n,
                                        self.accum_limit, self.light_groups.shape[0] * self.W * self.H, st)
            else:
                self.ctx.accumulate_tile(C.c_void_p(self.last_frame.data_ptr()), C.c_void_p(self.output.data_ptr()), n,
                                         self.accum_limit, st)
        if self.light_groups_denoised is not None:
            self._denoise_groups(st)
        self.last_params = (gp, p)
        return gp, p

    def _denoise_groups(self, st):
        """light_groups_denoised <- the frame's planes and output, denoised by one bmfr_execute_planes (the call is in/out:
        copies first)."""
        k = self.light_groups.shape[0]
        self.light_groups_denoised[:k].copy_(self.light_groups)
        self.light_groups_denoised[k].copy_(self.output)
        bp = abi.BmfrParams()
        bp.frameNumber, bp.flags = self.denoise_frame & 0xFFFFFFFF, self.denoise_flags
        vp = self._prev_view_proj if self._prev_view_proj is not None else [float(i % 5 == 0) for i in range(16)]
        for i in range(16):
            bp.prevViewProj[i] = vp[i]
        self.ctx.bmfr_execute_planes(bp, self.gb, self.light_groups_denoised, self.prev_position, st)
        self._prev_view_proj = view_proj_of_camera(self.cam)
        self.denoise_frame += 1
        self.last_denoise_params = bp

    def denoise_reset(self):
        """Forget the denoiser's history of the planes (after a cut): the next frame is its frame 0."""
        if self.light_groups_denoised is None:
            raise BdptError("denoise_reset: the pipeline does not denoise (FramePipeline(..., light_groups=..., denoise_groups=flags))")
        self.ctx.bmfr_planes_reset()
        self.denoise_frame = 0
        self._prev_view_proj = None

    def active_pixels(self):
        """Adaptive pipelines: pixels the next frame renders (the `active` word; waits for the pipeline's stream)."""
        if self.adaptive_state is None:
            raise BdptError("active_pixels: the pipeline is not adaptive (FramePipeline(..., adaptive={...}))")
        return int(self.adaptive_state["active"].item()) & 0xFFFFFFFF

    def adaptive_reset(self):
        """Adaptive pipelines: forget every pixel's mean and render all pixels again."""
        if self.adaptive_state is None:
            raise BdptError("adaptive_reset: the pipeline is not adaptive (FramePipeline(..., adaptive={...}))")
        self.ctx.adaptive_reset(self._adaptive_c, self._stream_ptr())

    def update_geometry(self, positions, normals=None, bitangents=None, keep_light_maps=False):
        """Move the scene's vertices (Context.update_geometry on this pipeline's stream); accumulation restarts, as after
        a camera move.  GPU tensors are marked as in use by that stream (the caching allocator does not hand their memory
        on before the stream has reached the update)."""
        self.ctx.update_geometry(positions, normals, bitangents, self._stream_ptr(), keep_light_maps)
        keep_for_stream(self.torch.cuda.current_stream(self.dev), (positions, normals, bitangents))
        self.accum_count = 0
        self._drop_restir_history()

    def set_skin(self, positions, bone_weights, bone_ids, num_bones, normals=None, bitangents=None):
        """Context.set_skin (synchronises: everything this pipeline enqueued has finished when it returns)."""
        self.ctx.set_skin(positions, bone_weights, bone_ids, num_bones, normals, bitangents)
        self._drop_restir_history()

    def update_skinned(self, bones, normal_bones=None, keep_light_maps=False):
        """Pose the skinned scene (Context.update_skinned on this pipeline's stream); accumulation restarts, as after
        update_geometry.  GPU tensors are marked as in use by that stream."""
        self.ctx.update_skinned(bones, normal_bones, self._stream_ptr(), keep_light_maps)
        keep_for_stream(self.torch.cuda.current_stream(self.dev), (bones, normal_bones))
        self.accum_count = 0
        self._drop_restir_history()

    def set_morph(self, target_start, vertex, d_positions, d_normals=None, d_bitangents=None, positions=None, normals=None,
                  bitangents=None):
        """Context.set_morph (synchronises: everything this pipeline enqueued has finished when it returns)."""
        self.ctx.set_morph(target_start, vertex, d_positions, d_normals, d_bitangents, positions, normals, bitangents)
        self._drop_restir_history()

    def update_morphed(self, weights, bones=None, normal_bones=None, keep_light_maps=False):
        """Morph (and pose) the scene (Context.update_morphed on this pipeline's stream); accumulation restarts, as after
        update_geometry.  GPU tensors are marked as in use by that stream."""
        self.ctx.update_morphed(weights, bones, normal_bones, self._stream_ptr(), keep_light_maps)
        keep_for_stream(self.torch.cuda.current_stream(self.dev), (weights, bones, normal_bones))
        self.accum_count = 0
        self._drop_restir_history()

    def trace_rays(self, rays, mode="closest", out=None, count=None):
        """Context.trace_rays on this pipeline's stream, ordered after its frames.  GPU tensors (rays, outputs, count) are
        marked as in use by that stream."""
        res = self.ctx.trace_rays(rays, mode, out, count, self._stream_ptr())
        outs = res if isinstance(res, tuple) else (res,)
        keep_for_stream(self.torch.cuda.current_stream(self.dev), (rays, count) + outs)
        return res

    def camera_rays(self, out=None):
        """Context.camera_rays with this pipeline's size and gbuffer_params() (the G-buffer pass's next frame: jitter and
        frame counter), on the pipeline's stream."""
        res = self.ctx.camera_rays(self.gbuffer_params(), self.W, self.H, out, self._stream_ptr())
        keep_for_stream(self.torch.cuda.current_stream(self.dev), (res,))
        return res

    def shade_hits(self, rays, hits, normal_map=True, out=None, count=None):
        """Context.shade_hits on this pipeline's stream, ordered after its frames."""
        res = self.ctx.shade_hits(rays, hits, normal_map, out, count, self._stream_ptr())
        keep_for_stream(self.torch.cuda.current_stream(self.dev), (rays, hits, count, res))
        return res

    def sample_bsdf(self, surfaces, seeds, from_lobe=None, out=None, count=None):
        """Context.sample_bsdf with the pipeline's BSDF (mat_index; from_lobe defaults to its SPECULAR_FROM_LOBE flag)."""
        if from_lobe is None:
            from_lobe = (self.flags & abi.PARAM_SPECULAR_FROM_LOBE) != 0
        res = self.ctx.sample_bsdf(surfaces, seeds, self.mat_index, from_lobe, out, count, self._stream_ptr())
        keep_for_stream(self.torch.cuda.current_stream(self.dev), (surfaces, seeds, count, res))
        return res

    def eval_bsdf(self, surfaces, dirs, out=None, count=None):
        """Context.eval_bsdf with the pipeline's BSDF (mat_index) on its stream."""
        res = self.ctx.eval_bsdf(surfaces, dirs, self.mat_index, out, count, self._stream_ptr())
        keep_for_stream(self.torch.cuda.current_stream(self.dev), (surfaces, dirs, count, res))
        return res

    def sample_lights(self, surfaces, seeds, use_hints=False, out=None, seeds_out=None, compact=None, count=None):
        """Context.sample_lights with the pipeline's BSDF (mat_index), min_t and PARAM_AREA_LIGHTS flag, on its stream."""
        res = self.ctx.sample_lights(surfaces, seeds, self.mat_index, self.min_t, (self.flags & abi.PARAM_AREA_LIGHTS) != 0, use_hints,
                                     out, seeds_out, compact, count, self._stream_ptr())
        keep_for_stream(self.torch.cuda.current_stream(self.dev), (surfaces, seeds, seeds_out, count, res) + tuple(compact or ()))
        return res

    def emit_lights(self, seeds, out=None, seeds_out=None, count=None):
        """Context.emit_lights with the pipeline's min_t and PARAM_AREA_LIGHTS flag, on its stream."""
        res = self.ctx.emit_lights(seeds, self.min_t, (self.flags & abi.PARAM_AREA_LIGHTS) != 0, out, seeds_out, count,
                                   self._stream_ptr())
        keep_for_stream(self.torch.cuda.current_stream(self.dev), (seeds, seeds_out, count, res))
        return res

    def connect_vertices(self, eye, light, eye_prev=None, light_prev=None, eye_specular=None, light_specular=None, out=None,
                         compact=None, count=None):
        """Context.connect_vertices with the pipeline's BSDF (mat_index) and min_t, on its stream."""
        res = self.ctx.connect_vertices(eye, light, self.mat_index, self.min_t, eye_prev, light_prev, eye_specular, light_specular,
                                        out, compact, count, self._stream_ptr())
        keep_for_stream(self.torch.cuda.current_stream(self.dev),
                        (eye, light, eye_prev, light_prev, eye_specular, light_specular, count, res) + tuple(compact or ()))
        return res

    def connect_camera(self, light, pixel_jitter=(0.0, 0.0), light_specular=None, out=None, compact=None, count=None):
        """Context.connect_camera with the pipeline's frame size, BSDF (mat_index) and min_t, on its stream.  pixel_jitter:
        the bdpt_params::pixelJitter of the frame the splats belong to."""
        res = self.ctx.connect_camera(light, self.W, self.H, pixel_jitter, self.mat_index, self.min_t, light_specular, out, compact,
                                      count, self._stream_ptr())
        keep_for_stream(self.torch.cuda.current_stream(self.dev), (light, light_specular, count, res) + tuple(compact or ()))
        return res

    def splat_add(self, splat, pixels, values, visible=None, items=None, count=None):
        """Context.splat_add on this pipeline's stream."""
        self.ctx.splat_add(splat, pixels, values, visible, items, count, self._stream_ptr())
        keep_for_stream(self.torch.cuda.current_stream(self.dev), (splat, pixels, values, visible, items, count))

    def walk(self, starts, seeds, steps, seed_per_step=False, first=None, first_specular=None, alive=None, out=None, samples=None,
             hits=None, count=None):
        """Context.walk with the pipeline's BSDF (mat_index), min_t and SPECULAR_FROM_LOBE flag, on its stream."""
        res = self.ctx.walk(starts, seeds, steps, self.mat_index, self.min_t, (self.flags & abi.PARAM_SPECULAR_FROM_LOBE) != 0,
                            seed_per_step, first, first_specular, alive, out, samples, hits, count, self._stream_ptr())
        keep_for_stream(self.torch.cuda.current_stream(self.dev),
                        (starts, seeds, first, first_specular, alive, samples, hits, count) + tuple(res))
        return res

    def motion_query(self, hits, out=None, count=None):
        """Context.motion_query on this pipeline's stream."""
        res = self.ctx.motion_query(hits, out, count, self._stream_ptr())
        keep_for_stream(self.torch.cuda.current_stream(self.dev), (hits, count, res))
        return res

    def _pass_channel(self, name):
        """The (H, W, 4) float32 channel a lighting pass writes, allocated (zeros) on first use."""
        if name not in self.channels:
            with self.torch.cuda.device(self.dev):
                self.channels[name] = self.torch.zeros(self.H, self.W, 4, dtype=self.torch.float32, device=self.dev)
        return self.channels[name]

    def ambient_occlusion(self, samples=1, radius=None):
        """The reference's AmbientOcclusionPass on this pipeline's G-buffer as it stands (render_frame, or a gbuffer_execute
        of the caller's, fills it) and stream: Context.ao_execute with the pass's frame counter (from 0, one per call:
        CommonPasses/AmbientOcclusionPass.h:54, .cpp:86), the pipeline's min_t and `samples` rays per pixel (1 .. 64; the pass's
        default 1).  radius=None is the pass's default for the scene, ao_default_radius.  Returns the (H, W, 4) float32
        channel "AmbientOcclusion" ((ao, ao, ao, 1); a tile or stripes pipeline writes its own rows), also in ``channels``;
        ``last_ao_params`` keeps the abi.AoParams used."""
        p = abi.AoParams()
        p.samples = Context._ao_samples("ambient_occlusion", samples)
        if radius is None:
            if self._ao_radius is None:  # once per pipeline, as the pass's initScene: the scene's vertices as loaded
                self._ao_radius = ao_default_radius(self.scene.desc)
            radius = self._ao_radius
        p.radius = float(radius)
        p.minT, p.frameCount = self.min_t, self.ao_frame & 0xFFFFFFFF
        out = self._pass_channel(AO_CHANNEL)
        self.ctx.ao_execute(p, self.gb, C.c_void_p(out.data_ptr()), self._stream_ptr())
        self.ao_frame += 1
        self.last_ao_params = p
        return out

    def sky_lighting(self, samples=1, clamp=float(3.4028234663852886e38), mis=False, mat_index=1):
        """Sky lighting on this pipeline's G-buffer as it stands and stream: Context.sky_execute with the pass's frame
        counter (from 0, one per call, as ambient_occlusion keeps its own), the pipeline's min_t, `samples` table-sampled rays
        per pixel (1 .. 64) and `clamp` as the bound of a sample's value.  With ``mis`` it is Context.sky_mis_execute: per
        sample a table-sampled and a BSDF-sampled ray, combined by the balance heuristic, for the Lambertian surface
        (``mat_index`` 1) or the pass's GGX material (0: MaterialSpecRough and the pipeline's camera are read as well);
        ``mat_index`` 0 without ``mis`` is refused.  The environment is the map given to
        ``ctx.set_environment``; its sampling table is prepared on first use and again whenever the environment was set anew
        through ``ctx.set_environment``.  The map's contents are not watched: after rewriting the map in place, call
        ``ctx.env_prepare`` (or set the environment again).
        Returns the (H, W, 4) float32 channel "SkyLighting" ((colour, 1); a tile or stripes pipeline writes its own rows),
        also in ``channels``; ``last_sky_params`` keeps the abi.SkyParams (abi.SkyMisParams with ``mis``) used."""
        mat_index, _ = Context._bsdf_mode("sky_lighting", mat_index, False)
        if not mis and mat_index != 1:
            raise BdptError("sky_lighting: mat_index 0 (GGX) goes with mis=True (the plain pass is Lambertian)")
        p = abi.SkyMisParams() if mis else abi.SkyParams()
        p.samples = Context._sky_samples("sky_lighting", samples)
        p.clampUpper = float(clamp)
        p.minT, p.frameCount = self.min_t, self.sky_frame & 0xFFFFFFFF
        if mis:
            p.matIndex, p.techniques = mat_index, abi.SKY_MIS_TABLE | abi.SKY_MIS_BSDF
        if self.ctx._env_prepared != self.ctx._env_serial:
            self.ctx.env_prepare(self._stream_ptr())
        out = self._pass_channel(SKY_CHANNEL)
        (self.ctx.sky_mis_execute if mis else self.ctx.sky_execute)(p, self.gb, C.c_void_p(out.data_ptr()), self._stream_ptr())
        self.sky_frame += 1
        self.last_sky_params = p
        return out

    def diffuse_gi(self, indirect=True, cosine=True):
        """The reference's SimpleDiffuseGIPass on this pipeline's G-buffer as it stands (render_frame, or a gbuffer_execute
        of the caller's, fills it) and stream: Context.gi_execute with the pass's frame counter (from 0x1337, one per call:
        CommonPasses/SimpleDiffuseGIPass.h:62, .cpp:100), the pipeline's min_t, camera and environment (Context.set_environment),
        and the pass's two switches (its defaults: indirect rays, cosine sampling).  Returns the (H, W, 4) float32 channel
        "DiffuseGI" ((colour, 1); a tile or stripes pipeline writes its own rows), also in ``channels``; ``last_gi_params``
        keeps the abi.GiParams used."""
        p = abi.GiParams()
        p.flags = (abi.GI_INDIRECT if indirect else 0) | (0 if cosine else abi.GI_UNIFORM)
        p.minT, p.frameCount = self.min_t, self.gi_frame & 0xFFFFFFFF
        out = self._pass_channel(GI_CHANNEL)
        self.ctx.gi_execute(p, self.gb, C.c_void_p(out.data_ptr()), self._stream_ptr())
        self.gi_frame += 1
        self.last_gi_params = p
        return out

    def direct_lighting(self, use_hints=False):
        """The reference's LambertianPlusShadowPass on this pipeline's G-buffer as it stands (render_frame, or a gbuffer_execute
        of the caller's, fills it) and stream: Context.direct_execute with the pipeline's min_t.  There is no frame counter:
        the pass draws nothing, so one call is converged direct lighting.  use_hints tries the lights' occluder hints first
        (the same image).  Returns the (H, W, 4) float32 channel "DirectLighting" ((colour, 1); a tile or stripes pipeline
        writes its own rows), also in ``channels``; ``last_direct_params`` keeps the abi.DirectParams used."""
        if not isinstance(use_hints, bool):
            raise BdptError(f"direct_lighting: use_hints must be a bool, not {use_hints!r}")
        out = self._pass_channel(DIRECT_CHANNEL)
        self.last_direct_params = self.ctx.direct_execute(self.gb, out, min_t=self.min_t, use_hints=use_hints, stream=self._stream_ptr())
        return out

    def ris_lighting(self, candidates, samples=1, mat_index=1, area_lights=False, use_hints=False,
                     clamp=float(3.4028234663852886e38)):
        """Resampled direct lighting on this pipeline's G-buffer as it stands and stream: Context.ris_execute with the pass's
        frame counter (from 0, one per call, as sky_lighting keeps its own), the pipeline's min_t, `candidates` next-event
        candidates (1 .. 32) and `samples` rays per pixel (1 .. 64), for the Lambertian surface (``mat_index`` 1) or the
        pass's GGX material (0: MaterialSpecRough and the pipeline's camera are read as well).  area_lights adds the
        emitter table as a candidate source, use_hints tries the lights' occluder hints first (the same image).  Returns
        the (H, W, 4) float32 channel "ResampledDirect" ((colour, 1); a tile or stripes pipeline writes its own rows), also
        in ``channels``; ``last_ris_params`` keeps the abi.RisParams used."""
        out = self._pass_channel(RIS_CHANNEL)
        self.last_ris_params = self.ctx.ris_execute(self.gb, out, candidates=candidates, samples=samples, mat_index=mat_index,
                                                    area_lights=area_lights, use_hints=use_hints, clamp=clamp, min_t=self.min_t,
                                                    frame_count=self.ris_frame, stream=self._stream_ptr())
        self.ris_frame += 1
        return out

    def restir_lighting(self, candidates, spatial=0, radius=8, temporal=False, max_m=None, mat_index=1, area_lights=False,
                        clamp=float(3.4028234663852886e38), normal_min=0.9, plane_max=float("inf")):
        """ReSTIR direct lighting on this pipeline's G-buffer as it stands and stream, one any-hit ray per pixel and pass:
        Context.ris_execute with `candidates` candidates, one sample and its reservoirs; with `temporal` and a history, a
        Context.reuse_execute whose one neighbour is the same pixel of last call's reservoirs, G-buffer copy and camera
        position; with `spatial` > 0, a Context.reuse_execute over that many neighbours at offsets drawn within `radius`.
        A pool reservoir counts for at most `max_m` candidates (default 20 * candidates); neighbours must pass normal_min and
        plane_max.  The pass's frame counter (from 0, one per call) seeds the first stage; the temporal pass runs at twice
        that count and the spatial pass at twice plus one, so no two passes share a stream.  The last pass's reservoirs,
        the G-buffer and the camera position become the history of the next call; set_lights and every geometry update drop
        it, since a history's samples are re-evaluated with the current lights.  Returns the (H, W, 4) float32 channel
        "RestirDirect", also in ``channels``.  A tile or stripes pipeline raises BdptError: ranks do not exchange
        reservoirs."""
        torch = self.torch
        if self.stripes is not None or (self.y0, self.y1) != (0, self.H):
            raise BdptError("restir_lighting: a tile or stripes pipeline cannot reuse reservoirs (its neighbours and history lie on other ranks)")
        for name, v, top in (("spatial", spatial, abi.REUSE_MAX_NEIGHBORS), ("radius", radius, abi.REUSE_MAX_RADIUS)):
            if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= top:
                raise BdptError(f"restir_lighting: {name} must be an integer in 0 .. {top}, not {v!r}")
        if not isinstance(temporal, bool):
            raise BdptError(f"restir_lighting: temporal must be a bool, not {temporal!r}")
        candidates, _, _, _, clamp = Context._ris_mode("restir_lighting", candidates, 1, mat_index, area_lights, False, clamp)
        max_m = 20 * candidates if max_m is None else max_m
        if isinstance(max_m, bool) or not isinstance(max_m, int) or not 1 <= max_m < 2**32:
            raise BdptError(f"restir_lighting: max_m must be an integer in 1 .. 2^32 - 1, not {max_m!r}")
        if spatial and radius < 1:
            raise BdptError("restir_lighting: spatial neighbours need a radius of at least 1")
        out = self._pass_channel(RESTIR_CHANNEL)
        st = self._restir
        if st is None:
            with torch.cuda.device(self.dev):
                st = self._restir = dict(
                    res=[torch.zeros(self.H, self.W, 4, dtype=torch.int32, device=self.dev) for _ in range(4)],  # history, and one per pass
                    channels=[torch.zeros_like(self.channels[n]) for n in GBUFFER_CHANNELS[:4]], cam=(0.0, 0.0, 0.0), valid=False,
                    m=0)  # m: the candidate count of every history record; 0: the records' M words (a reuse pass wrote them)
                st["gb"] = GBuffer(*([t.data_ptr() for t in st["channels"]] + [None, None]))
        hist, first, second, third = st["res"]
        frame, stream = self.restir_frame, self._stream_ptr()
        cam = tuple(float(v) for v in self.cam.posW)
        common = dict(mat_index=mat_index, area_lights=area_lights, clamp=clamp, min_t=self.min_t, stream=stream)
        self.ctx.ris_execute(self.gb, out, candidates=candidates, samples=1, frame_count=frame, reservoirs=first.view(self.H, self.W, 1, 4),
                             **common)
        cur, in_m = first, candidates
        if temporal and st["valid"]:
            self.ctx.reuse_execute(self.gb, out, cur, neighbors=1, same_pixel=True, pool_gbuffer=st["gb"], pool_reservoirs=hist,
                                   pool_camera_pos=st["cam"], in_m=in_m, pool_m=st["m"], max_m=max_m, normal_min=normal_min, plane_max=plane_max,
                                   frame_count=2 * frame, reservoirs_out=second, **common)
            cur, in_m = second, 0
        if spatial:
            self.ctx.reuse_execute(self.gb, out, cur, neighbors=spatial, radius=radius, pool_camera_pos=cam, in_m=in_m, pool_m=in_m, max_m=max_m,
                                   normal_min=normal_min, plane_max=plane_max, frame_count=2 * frame + 1, reservoirs_out=third, **common)
            cur, in_m = third, 0
        # The history of the next call.  A background pixel's record may be stale (the first stage does not write it): a
        # dead pool pixel is rejected before its record is read, which holds as long as these copies are made together.
        hist.copy_(cur)
        for dst, name in zip(st["channels"], GBUFFER_CHANNELS[:4]):
            dst.copy_(self.channels[name])
        st["cam"], st["valid"], st["m"] = cam, True, in_m  # (a first stage's records end in wsum: their count is the call's)
        self.restir_frame += 1
        return out

    def _drop_restir_history(self):
        if self._restir is not None:
            self._restir["valid"] = False

    def set_lights(self, lights):
        """Move the scene's lights (Context.set_lights on this pipeline's stream); accumulation restarts."""
        self.ctx.set_lights(lights, self._stream_ptr())
        self.accum_count = 0
        self._drop_restir_history()

    def close(self):
        self.ctx.close()
