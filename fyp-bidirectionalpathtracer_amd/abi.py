"""ctypes view of include/bdpt.h and include/bdpt_scene.h.

Plumbing only: struct layouts, prototypes and the loader for the in-tree
``libbdpt_amd.so``.  There is no CPU fallback — if the library is missing or was
built without its HIP kernels, loading fails loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libbdpt_amd.so")

BDPT_MAX_DEPTH = 16
BDPT_MAX_LIGHTS = 16
PARAM_COUNTERS = 1
PARAM_DEFER_RESOLVE = 2
PARAM_NO_NEE = 4
PARAM_NO_SPLAT = 8
PARAM_NO_CONNECT = 16
PARAM_SPECULAR_FROM_LOBE = 32
PARAM_MIS_POWER = 64
PARAM_MIS_LINEAR = 128
PARAM_DEFER_TAIL = 256
PARAM_KEEP_COUNTERS = 512
PARAM_ENV_ON_MISS = 1024
PARAM_EMISSIVE_HITS = 2048
PARAM_AREA_LIGHTS = 4096
PREPARE_PRIMARY = 1
PREPARE_BMFR = 2
PREPARE_REFIT = 4
PREPARE_LIGHT_GROUPS = 8
PREPARE_AREA_LIGHTS = 16
PREPARE_LIGHT_GROUP_TABLE = 32
PREPARE_MOTION = 64
PREPARE_REFIT_PIECES = 128
MEMORY_HOST, MEMORY_DEVICE = 0, 1
UPDATE_KEEP_LIGHT_MAPS = 1
BDPT_MAX_BONES = 1024
MAX_MORPH_TARGETS = 1024
# csrc/skin.h kSkinLdsBones / kSkinLdsMinVertices: palettes up to this size on skins of at least this many vertices take the
# kernel's LDS path
SKIN_LDS_BONES, SKIN_LDS_MIN_VERTICES = 64, 1 << 20
SKIN_PATH_AUTO, SKIN_PATH_GLOBAL, SKIN_PATH_LDS = 0, 1, 2
# bdpt_test_morph_kernel: the same paths, chosen by the same rule (csrc/morph.h launchDeform)
MORPH_PATH_AUTO, MORPH_PATH_GLOBAL, MORPH_PATH_LDS = 0, 1, 2
TRACE_CLOSEST, TRACE_CLOSEST_CULL_BACK, TRACE_ANY = 0, 1, 2
SHADE_NORMAL_MAP = 1
BSDF_SAMPLE, BSDF_EVAL = 0, 1
LIGHT_NEE, LIGHT_EMIT = 0, 1
LIGHT_USE_HINTS = 1
LIGHT_STATUS_NONZERO, LIGHT_STATUS_HINT_OCCLUDED = 1, 2
CONNECT_VERTICES, CONNECT_CAMERA = 0, 1
CONNECT_STATUS_NONZERO, CONNECT_STATUS_PIXEL = 1, 2
WALK_SEED_PER_STEP = 1
WALK_STATUS_STORED, WALK_STATUS_REAL, WALK_STATUS_SPECULAR = 1, 2, 4
AO_MAX_SAMPLES = 64
GI_INDIRECT, GI_UNIFORM, GI_SHADE_FROM_VIEW = 1, 2, 4
GI_STATUS_DIRECT_OCCLUDED, GI_STATUS_BOUNCE_HIT, GI_STATUS_BOUNCE_OCCLUDED = 1, 2, 4
DIRECT_USE_HINTS = 1


class Material(C.Structure):
    _fields_ = [("baseColor", C.c_float * 4), ("specular", C.c_float * 4), ("emissive", C.c_float * 3),
                ("alphaThreshold", C.c_float), ("IoR", C.c_float), ("flags", C.c_uint32),
                ("texBaseColor", C.c_int16), ("texSpecular", C.c_int16), ("texEmissive", C.c_int16),
                ("texNormal", C.c_int16)]


class Texture(C.Structure):
    _fields_ = [("rgba8", C.POINTER(C.c_uint8)), ("width", C.c_uint32), ("height", C.c_uint32),
                ("srgb", C.c_uint32), ("reserved", C.c_uint32)]


class Light(C.Structure):
    _fields_ = [("posW", C.c_float * 3), ("type", C.c_uint32), ("dirW", C.c_float * 3),
                ("openingAngle", C.c_float), ("intensity", C.c_float * 3), ("cosOpeningAngle", C.c_float),
                ("penumbraAngle", C.c_float), ("reserved", C.c_float * 3)]


LIGHT_POINT, LIGHT_DIRECTIONAL = 0, 1
BMFR_PREPROCESS, BMFR_REGRESSION, BMFR_POSTPROCESS, BMFR_KEEP_LD_FEATURES, BMFR_FULL_FRAME = 1, 2, 4, 8, 16


class BmfrParams(C.Structure):
    _fields_ = [("frameNumber", C.c_uint32), ("flags", C.c_uint32), ("prevViewProj", C.c_float * 16)]


class SceneDesc(C.Structure):
    _fields_ = [("numVertices", C.c_uint32), ("numTriangles", C.c_uint32), ("numMaterials", C.c_uint32),
                ("numTextures", C.c_uint32), ("numLights", C.c_uint32), ("reserved", C.c_uint32),
                ("positions", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)),
                ("bitangents", C.POINTER(C.c_float)), ("texcoords", C.POINTER(C.c_float)),
                ("indices", C.POINTER(C.c_uint32)), ("triMaterial", C.POINTER(C.c_uint32)),
                ("materials", C.POINTER(Material)), ("textures", C.POINTER(Texture)),
                ("lights", C.POINTER(Light))]


class Camera(C.Structure):
    _fields_ = [("posW", C.c_float * 3), ("cameraU", C.c_float * 3), ("cameraV", C.c_float * 3),
                ("cameraW", C.c_float * 3)]


class Params(C.Structure):
    _fields_ = [("minT", C.c_float), ("frameCount", C.c_uint32), ("matIndex", C.c_uint32),
                ("refractiveIndex", C.c_float), ("maxDepth", C.c_uint32), ("emitMult", C.c_float),
                ("clampUpper", C.c_float), ("pixelJitter", C.c_float * 2), ("flags", C.c_uint32)]


class GBufferParams(C.Structure):
    _fields_ = [("pixelJitter", C.c_float * 2), ("lensRadius", C.c_float), ("focalLen", C.c_float),
                ("frameCount", C.c_uint32), ("useThinLens", C.c_uint32), ("envWidth", C.c_uint32),
                ("envHeight", C.c_uint32), ("envMap", C.c_void_p), ("envColor", C.c_float * 4)]


class GBuffer(C.Structure):
    _fields_ = [("worldPosition", C.c_void_p), ("worldNormal", C.c_void_p), ("materialDiffuse", C.c_void_p),
                ("materialSpecRough", C.c_void_p), ("materialExtraParams", C.c_void_p), ("emissive", C.c_void_p)]


class Tile(C.Structure):
    _fields_ = [("y0", C.c_uint32), ("y1", C.c_uint32)]


class Stripes(C.Structure):
    _fields_ = [("stripeRows", C.c_uint32), ("numOwners", C.c_uint32), ("owner", C.c_uint32)]


class TileInfo(C.Structure):
    _fields_ = [("numRows", C.c_uint32), ("numPixels", C.c_uint32), ("chunkRows", C.c_uint32), ("numRowRanges", C.c_uint32),
                ("splatU64", C.c_uint64), ("chunkU64", C.c_uint64)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "raysPrimary", "raysEyeExtend", "raysLightExtend", "raysNee", "raysSplat", "raysConnect",
        "nodeVisitsClosest", "triTestsClosest", "nodeVisitsShadow", "triTestsShadow", "pixelsValid",
        "splatsLanded", "raysConnectLazy", "alphaTestsClosest", "alphaTestsShadow", "hintedNee", "hintedSplat")]

    def total_rays(self):
        return (self.raysPrimary + self.raysEyeExtend + self.raysLightExtend + self.raysNee + self.raysSplat +
                self.raysConnect)

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class Environment(C.Structure):
    _fields_ = [("envMap", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("color", C.c_float * 4)]


class BvhInfo(C.Structure):
    _fields_ = [("numNodes", C.c_uint32), ("numTriangles", C.c_uint32), ("maxDepth", C.c_uint32),
                ("nodeBytes", C.c_uint32), ("triBytes", C.c_uint32), ("sahCost", C.c_float), ("maxStack", C.c_uint32),
                ("reserved", C.c_uint32), ("numReferences", C.c_uint32), ("numDropped", C.c_uint32),
                ("numAlphaMode", C.c_uint32), ("numAlwaysPass", C.c_uint32)]


class GeometryUpdate(C.Structure):
    _fields_ = [("positions", C.c_void_p), ("normals", C.c_void_p), ("bitangents", C.c_void_p), ("numVertices", C.c_uint32),
                ("memory", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class SkinDesc(C.Structure):
    _fields_ = [("numVertices", C.c_uint32), ("numBones", C.c_uint32), ("positions", C.c_void_p), ("normals", C.c_void_p),
                ("bitangents", C.c_void_p), ("boneWeights", C.c_void_p), ("boneIds", C.c_void_p), ("reserved", C.c_uint32 * 2)]


class SkinUpdate(C.Structure):
    _fields_ = [("bones", C.c_void_p), ("normalBones", C.c_void_p), ("numBones", C.c_uint32), ("memory", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class MorphDesc(C.Structure):
    _fields_ = [("numVertices", C.c_uint32), ("numTargets", C.c_uint32), ("targetStart", C.c_void_p), ("vertex", C.c_void_p),
                ("dPositions", C.c_void_p), ("dNormals", C.c_void_p), ("dBitangents", C.c_void_p), ("positions", C.c_void_p),
                ("normals", C.c_void_p), ("bitangents", C.c_void_p), ("reserved", C.c_uint32 * 2)]


class MorphUpdate(C.Structure):
    _fields_ = [("weights", C.c_void_p), ("bones", C.c_void_p), ("normalBones", C.c_void_p), ("numTargets", C.c_uint32),
                ("numBones", C.c_uint32), ("memory", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class RefitInfo(C.Structure):
    _fields_ = [("sahCost", C.c_float), ("sahCostBuilt", C.c_float), ("numUpdates", C.c_uint32), ("reserved", C.c_uint32)]


class Ray(C.Structure):
    _fields_ = [("org", C.c_float * 3), ("tmin", C.c_float), ("dir", C.c_float * 3), ("tmax", C.c_float)]


class Hit(C.Structure):
    _fields_ = [("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("prim", C.c_int32)]


class AdaptiveState(C.Structure):
    _fields_ = [("mean", C.c_void_p), ("m2", C.c_void_p), ("count", C.c_void_p), ("mask", C.c_void_p), ("active", C.c_void_p)]


class AdaptiveParams(C.Structure):
    _fields_ = [("threshold", C.c_float), ("epsilon", C.c_float), ("minSamples", C.c_uint32), ("maxSamples", C.c_uint32),
                ("blockSize", C.c_uint32)]


class TraceDesc(C.Structure):
    _fields_ = [("rays", C.c_void_p), ("numRays", C.c_uint32), ("mode", C.c_uint32), ("numRaysDevice", C.c_void_p),
                ("hits", C.c_void_p), ("visible", C.c_void_p)]


class Surface(C.Structure):
    _fields_ = [("posW", C.c_float * 3), ("dist", C.c_float), ("N", C.c_float * 3), ("linearRoughness", C.c_float),
                ("V", C.c_float * 3), ("IoR", C.c_float), ("diffuse", C.c_float * 3), ("opacity", C.c_float),
                ("specular", C.c_float * 3), ("material", C.c_uint32), ("emissive", C.c_float * 3), ("prim", C.c_int32)]


class ShadeDesc(C.Structure):
    _fields_ = [("rays", C.c_void_p), ("hits", C.c_void_p), ("numHits", C.c_uint32), ("flags", C.c_uint32),
                ("numHitsDevice", C.c_void_p), ("surfaces", C.c_void_p)]


class MotionDesc(C.Structure):
    _fields_ = [("hits", C.c_void_p), ("num", C.c_uint32), ("reserved", C.c_uint32), ("numDevice", C.c_void_p),
                ("prevPositions", C.c_void_p)]


class BsdfSample(C.Structure):
    _fields_ = [("dir", C.c_float * 3), ("pdf", C.c_float), ("weight", C.c_float * 3), ("specular", C.c_uint32)]


class BsdfDesc(C.Structure):
    _fields_ = [("surfaces", C.c_void_p), ("num", C.c_uint32), ("mode", C.c_uint32), ("numDevice", C.c_void_p),
                ("matIndex", C.c_uint32), ("flags", C.c_uint32), ("seeds", C.c_void_p), ("samples", C.c_void_p),
                ("dirs", C.c_void_p), ("values", C.c_void_p)]


class LightSample(C.Structure):
    _fields_ = [("ray", Ray), ("value", C.c_float * 3), ("light", C.c_uint16), ("status", C.c_uint16)]


class LightEmit(C.Structure):
    _fields_ = [("ray", Ray), ("color", C.c_float * 3), ("light", C.c_uint32)]


class LightDesc(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("num", C.c_uint32), ("numDevice", C.c_void_p), ("matIndex", C.c_uint32),
                ("flags", C.c_uint32), ("minT", C.c_float), ("reserved", C.c_uint32), ("surfaces", C.c_void_p),
                ("seeds", C.c_void_p), ("seedsOut", C.c_void_p), ("samples", C.c_void_p), ("emits", C.c_void_p),
                ("compactRays", C.c_void_p), ("compactItems", C.c_void_p), ("compactCount", C.c_void_p)]


class ConnectSample(C.Structure):
    _fields_ = [("ray", Ray), ("value", C.c_float * 3), ("status", C.c_uint32)]


class CameraSample(C.Structure):
    _fields_ = [("ray", Ray), ("f", C.c_float * 3), ("G", C.c_float), ("pixel", C.c_uint32), ("status", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]


class ConnectDesc(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("num", C.c_uint32), ("numDevice", C.c_void_p), ("matIndex", C.c_uint32),
                ("flags", C.c_uint32), ("minT", C.c_float), ("reserved", C.c_uint32), ("eye", C.c_void_p), ("light", C.c_void_p),
                ("eyePrev", C.c_void_p), ("lightPrev", C.c_void_p), ("eyeSpecular", C.c_void_p), ("lightSpecular", C.c_void_p),
                ("samples", C.c_void_p), ("cameraSamples", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32),
                ("pixelJitter", C.c_float * 2), ("compactRays", C.c_void_p), ("compactItems", C.c_void_p),
                ("compactCount", C.c_void_p)]


class SplatDesc(C.Structure):
    _fields_ = [("num", C.c_uint32), ("numPixels", C.c_uint32), ("numDevice", C.c_void_p), ("pixels", C.c_void_p),
                ("values", C.c_void_p), ("visible", C.c_void_p), ("items", C.c_void_p), ("splat", C.c_void_p)]


class WalkStart(C.Structure):
    _fields_ = [("ray", Ray), ("color", C.c_float * 3), ("unused", C.c_uint32)]


class WalkInfo(C.Structure):
    _fields_ = [("color", C.c_float * 3), ("status", C.c_uint32)]


class WalkDesc(C.Structure):
    _fields_ = [("num", C.c_uint32), ("steps", C.c_uint32), ("numDevice", C.c_void_p), ("matIndex", C.c_uint32),
                ("flags", C.c_uint32), ("minT", C.c_float), ("reserved", C.c_uint32), ("starts", C.c_void_p), ("seeds", C.c_void_p),
                ("first", C.c_void_p), ("firstSpecular", C.c_void_p), ("alive", C.c_void_p), ("vertices", C.c_void_p),
                ("info", C.c_void_p), ("samples", C.c_void_p), ("hits", C.c_void_p)]


class AoDesc(C.Structure):
    _fields_ = [("num", C.c_uint32), ("samples", C.c_uint32), ("numDevice", C.c_void_p), ("radius", C.c_float), ("minT", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_uint32), ("surfaces", C.c_void_p), ("seeds", C.c_void_p), ("alive", C.c_void_p),
                ("ao", C.c_void_p), ("counts", C.c_void_p), ("seedsOut", C.c_void_p)]


class AoParams(C.Structure):
    _fields_ = [("frameCount", C.c_uint32), ("radius", C.c_float), ("minT", C.c_float), ("samples", C.c_uint32),
                ("reserved", C.c_uint32)]


class GiDesc(C.Structure):
    _fields_ = [("num", C.c_uint32), ("flags", C.c_uint32), ("numDevice", C.c_void_p), ("shadeFlags", C.c_uint32), ("minT", C.c_float),
                ("viewPos", C.c_float * 3), ("reserved", C.c_uint32), ("surfaces", C.c_void_p), ("seeds", C.c_void_p),
                ("alive", C.c_void_p), ("color", C.c_void_p), ("hits", C.c_void_p), ("status", C.c_void_p), ("seedsOut", C.c_void_p)]


class GiParams(C.Structure):
    _fields_ = [("frameCount", C.c_uint32), ("minT", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class DirectDesc(C.Structure):
    _fields_ = [("num", C.c_uint32), ("flags", C.c_uint32), ("numDevice", C.c_void_p), ("minT", C.c_float), ("reserved", C.c_uint32),
                ("surfaces", C.c_void_p), ("alive", C.c_void_p), ("color", C.c_void_p), ("visible", C.c_void_p),
                ("traced", C.c_void_p)]


class DirectParams(C.Structure):
    _fields_ = [("minT", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


ENV_MAX_DIM = 16384
ENV_SAMPLE, ENV_EVAL = 0, 1
ENV_STATUS_NONZERO = 1
SKY_MAX_SAMPLES = 64
ENV_NO_TEXEL = 0xFFFFFFFF
# texels per pass of the table's row scan and rows per pass of its marginal scan (csrc/env_light.h; bdpt_get_env_info
# reports them): sizes just past them cross a carry
ENV_ROW_SCAN_CHUNK, ENV_MARGINAL_CHUNK = 64, 64


class EnvInfo(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("total", C.c_uint64), ("max", C.c_float),
                ("rowScanChunk", C.c_uint32), ("marginalChunk", C.c_uint32), ("reserved", C.c_uint32), ("tableBytes", C.c_uint64),
                ("cdf", C.c_void_p), ("rowCdf", C.c_void_p)]


class EnvSample(C.Structure):
    _fields_ = [("ray", Ray), ("radiance", C.c_float * 3), ("pdf", C.c_float), ("value", C.c_float * 3), ("texel", C.c_uint32),
                ("status", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class EnvEval(C.Structure):
    _fields_ = [("radiance", C.c_float * 3), ("pdf", C.c_float), ("texel", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class EnvHostSample(C.Structure):
    _fields_ = [("dir", C.c_float * 3), ("pdf", C.c_float), ("radiance", C.c_float * 3), ("texel", C.c_uint32)]


class EnvDesc(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("num", C.c_uint32), ("numDevice", C.c_void_p), ("matIndex", C.c_uint32), ("flags", C.c_uint32),
                ("minT", C.c_float), ("reserved", C.c_uint32), ("surfaces", C.c_void_p), ("seeds", C.c_void_p), ("seedsOut", C.c_void_p),
                ("samples", C.c_void_p), ("dirs", C.c_void_p), ("evals", C.c_void_p), ("compactRays", C.c_void_p),
                ("compactItems", C.c_void_p), ("compactCount", C.c_void_p)]


class SkyDesc(C.Structure):
    _fields_ = [("num", C.c_uint32), ("samples", C.c_uint32), ("numDevice", C.c_void_p), ("clampUpper", C.c_float), ("minT", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_uint32), ("surfaces", C.c_void_p), ("seeds", C.c_void_p), ("alive", C.c_void_p),
                ("color", C.c_void_p), ("counts", C.c_void_p), ("seedsOut", C.c_void_p)]


class SkyParams(C.Structure):
    _fields_ = [("frameCount", C.c_uint32), ("clampUpper", C.c_float), ("minT", C.c_float), ("samples", C.c_uint32),
                ("reserved", C.c_uint32)]


SKY_MIS_TABLE, SKY_MIS_BSDF = 1, 2  # bdpt_sky_mis_desc::techniques


class BsdfPdfDesc(C.Structure):
    _fields_ = [("num", C.c_uint32), ("matIndex", C.c_uint32), ("numDevice", C.c_void_p), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("surfaces", C.c_void_p), ("dirs", C.c_void_p), ("values", C.c_void_p)]


class SkyMisDesc(C.Structure):
    _fields_ = [("num", C.c_uint32), ("samples", C.c_uint32), ("numDevice", C.c_void_p), ("clampUpper", C.c_float), ("minT", C.c_float),
                ("matIndex", C.c_uint32), ("techniques", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("surfaces", C.c_void_p), ("seeds", C.c_void_p), ("alive", C.c_void_p), ("color", C.c_void_p), ("counts", C.c_void_p),
                ("seedsOut", C.c_void_p)]


class SkyMisParams(C.Structure):
    _fields_ = [("frameCount", C.c_uint32), ("clampUpper", C.c_float), ("minT", C.c_float), ("samples", C.c_uint32),
                ("matIndex", C.c_uint32), ("techniques", C.c_uint32), ("reserved", C.c_uint32 * 2)]


RIS_USE_HINTS = 1  # bdpt_ris_desc::flags, beside PARAM_AREA_LIGHTS
RIS_MAX_CANDIDATES, RIS_MAX_SAMPLES = 32, 64
RIS_STATUS_RAY, RIS_STATUS_HINT_OCCLUDED, RIS_STATUS_OCCLUDED = 1, 2, 4  # bdpt_ris_reservoir::status
RIS_NO_LIGHT = 0xFFFF


class RisReservoir(C.Structure):
    _fields_ = [("light", C.c_uint16), ("status", C.c_uint16), ("state", C.c_uint32), ("W", C.c_float), ("wsum", C.c_float)]


class RisDesc(C.Structure):
    _fields_ = [("num", C.c_uint32), ("flags", C.c_uint32), ("numDevice", C.c_void_p), ("matIndex", C.c_uint32),
                ("candidates", C.c_uint32), ("samples", C.c_uint32), ("clampUpper", C.c_float), ("minT", C.c_float),
                ("reserved", C.c_uint32), ("surfaces", C.c_void_p), ("alive", C.c_void_p), ("seeds", C.c_void_p),
                ("color", C.c_void_p), ("seedsOut", C.c_void_p), ("traced", C.c_void_p), ("reservoirs", C.c_void_p)]


class RisParams(C.Structure):
    _fields_ = [("frameCount", C.c_uint32), ("clampUpper", C.c_float), ("minT", C.c_float), ("candidates", C.c_uint32),
                ("samples", C.c_uint32), ("matIndex", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


REUSE_MAX_NEIGHBORS, REUSE_MAX_M = 8, 1 << 24
REUSE_SAME_PIXEL = 1  # bdpt_reuse_params::flags, beside PARAM_AREA_LIGHTS
REUSE_MAX_RADIUS = 1024


class ReuseReservoir(C.Structure):
    _fields_ = [("light", C.c_uint16), ("status", C.c_uint16), ("state", C.c_uint32), ("W", C.c_float), ("M", C.c_uint32)]


class ReuseDesc(C.Structure):
    _fields_ = [("num", C.c_uint32), ("flags", C.c_uint32), ("numDevice", C.c_void_p), ("matIndex", C.c_uint32),
                ("neighbors", C.c_uint32), ("inM", C.c_uint32), ("poolM", C.c_uint32), ("maxM", C.c_uint32), ("poolNum", C.c_uint32),
                ("normalMin", C.c_float), ("planeMax", C.c_float), ("clampUpper", C.c_float), ("minT", C.c_float),
                ("reserved", C.c_uint32 * 2), ("surfaces", C.c_void_p), ("alive", C.c_void_p), ("seeds", C.c_void_p),
                ("in", C.c_void_p), ("poolSurfaces", C.c_void_p), ("poolAlive", C.c_void_p), ("pool", C.c_void_p),
                ("neighborIndex", C.c_void_p), ("color", C.c_void_p), ("seedsOut", C.c_void_p), ("traced", C.c_void_p),
                ("out", C.c_void_p)]  # `in` is a Python keyword: setattr(desc, "in", pointer)


class ReuseParams(C.Structure):
    _fields_ = [("frameCount", C.c_uint32), ("clampUpper", C.c_float), ("minT", C.c_float), ("matIndex", C.c_uint32),
                ("flags", C.c_uint32), ("neighbors", C.c_uint32), ("radius", C.c_uint32), ("inM", C.c_uint32), ("poolM", C.c_uint32),
                ("maxM", C.c_uint32), ("normalMin", C.c_float), ("planeMax", C.c_float), ("poolCameraPos", C.c_float * 3),
                ("reserved", C.c_uint32), ("in", C.c_void_p), ("poolGbuffer", C.POINTER(GBuffer)), ("pool", C.c_void_p),
                ("neighborIndex", C.c_void_p), ("outReservoirs", C.c_void_p)]


BMFR_MAX_PLANES = BDPT_MAX_LIGHTS + 2


class BmfrPlanesDesc(C.Structure):
    _fields_ = [("planes", C.POINTER(C.c_void_p)), ("numPlanes", C.c_uint32), ("reserved", C.c_uint32),
                ("prevPosition", C.c_void_p)]


class LightGroupDesc(C.Structure):
    _fields_ = [("planes", C.c_void_p), ("numGroups", C.c_uint32), ("numAssigned", C.c_uint32),
                ("groupOf", C.POINTER(C.c_uint8)), ("reserved", C.c_uint32 * 2)]


class AreaLightInfo(C.Structure):
    _fields_ = [("numEmitters", C.c_uint32), ("numTextured", C.c_uint32), ("totalWeight", C.c_float), ("reserved", C.c_uint32)]


# name -> (restype, argtypes); every symbol include/*.h declares
PROTOTYPES = {
    "bdpt_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "bdpt_destroy": (None, [C.c_void_p]),
    "bdpt_last_error": (C.c_char_p, [C.c_void_p]),
    "bdpt_set_scene": (C.c_int, [C.c_void_p, C.POINTER(SceneDesc)]),
    "bdpt_get_bvh_info": (C.c_int, [C.c_void_p, C.POINTER(BvhInfo)]),
    "bdpt_set_camera": (C.c_int, [C.c_void_p, C.POINTER(Camera)]),
    "bdpt_set_environment": (C.c_int, [C.c_void_p, C.POINTER(Environment)]),
    "bdpt_bvh_build_check": (C.c_int, [C.POINTER(SceneDesc), C.POINTER(BvhInfo), C.c_char_p, C.c_uint32]),
    "bdpt_host_bvh_create": (C.c_void_p, [C.POINTER(SceneDesc), C.c_int, C.c_float, C.c_float, C.c_int, C.POINTER(BvhInfo)]),
    "bdpt_host_bvh_destroy": (None, [C.c_void_p]),
    "bdpt_host_bvh_trace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "bdpt_update_geometry": (C.c_int, [C.c_void_p, C.POINTER(GeometryUpdate), C.c_void_p]),
    "bdpt_set_lights": (C.c_int, [C.c_void_p, C.POINTER(Light), C.c_uint32, C.c_void_p]),
    "bdpt_get_refit_info": (C.c_int, [C.c_void_p, C.POINTER(RefitInfo)]),
    "bdpt_set_skin": (C.c_int, [C.c_void_p, C.POINTER(SkinDesc)]),
    "bdpt_update_skinned": (C.c_int, [C.c_void_p, C.POINTER(SkinUpdate), C.c_void_p]),
    "bdpt_skinned_buffers": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "bdpt_host_skin": (C.c_int, [C.POINTER(SkinDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bdpt_test_skin_kernel": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "bdpt_set_morph": (C.c_int, [C.c_void_p, C.POINTER(MorphDesc)]),
    "bdpt_update_morphed": (C.c_int, [C.c_void_p, C.POINTER(MorphUpdate), C.c_void_p]),
    "bdpt_morphed_buffers": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "bdpt_host_morph": (C.c_int, [C.POINTER(MorphDesc), C.POINTER(SkinDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "bdpt_test_morph_kernel": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "bdpt_trace_rays": (C.c_int, [C.c_void_p, C.POINTER(TraceDesc), C.c_void_p]),
    "bdpt_camera_rays": (C.c_int, [C.c_void_p, C.POINTER(GBufferParams), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "bdpt_shade_hits": (C.c_int, [C.c_void_p, C.POINTER(ShadeDesc), C.c_void_p]),
    "bdpt_bsdf_query": (C.c_int, [C.c_void_p, C.POINTER(BsdfDesc), C.c_void_p]),
    "bdpt_keep_pose": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bdpt_motion_query": (C.c_int, [C.c_void_p, C.POINTER(MotionDesc), C.c_void_p]),
    "bdpt_light_query": (C.c_int, [C.c_void_p, C.POINTER(LightDesc), C.c_void_p]),
    "bdpt_connect_query": (C.c_int, [C.c_void_p, C.POINTER(ConnectDesc), C.c_void_p]),
    "bdpt_splat_add": (C.c_int, [C.c_void_p, C.POINTER(SplatDesc), C.c_void_p]),
    "bdpt_walk_query": (C.c_int, [C.c_void_p, C.POINTER(WalkDesc), C.c_void_p]),
    "bdpt_ao_query": (C.c_int, [C.c_void_p, C.POINTER(AoDesc), C.c_void_p]),
    "bdpt_ao_execute": (C.c_int, [C.c_void_p, C.POINTER(AoParams), C.POINTER(GBuffer), C.c_void_p, C.c_void_p]),
    "bdpt_gi_query": (C.c_int, [C.c_void_p, C.POINTER(GiDesc), C.c_void_p]),
    "bdpt_gi_execute": (C.c_int, [C.c_void_p, C.POINTER(GiParams), C.POINTER(GBuffer), C.c_void_p, C.c_void_p]),
    "bdpt_direct_query": (C.c_int, [C.c_void_p, C.POINTER(DirectDesc), C.c_void_p]),
    "bdpt_direct_execute": (C.c_int, [C.c_void_p, C.POINTER(DirectParams), C.POINTER(GBuffer), C.c_void_p, C.c_void_p]),
    "bdpt_env_prepare": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bdpt_get_env_info": (C.c_int, [C.c_void_p, C.POINTER(EnvInfo)]),
    "bdpt_env_query": (C.c_int, [C.c_void_p, C.POINTER(EnvDesc), C.c_void_p]),
    "bdpt_sky_query": (C.c_int, [C.c_void_p, C.POINTER(SkyDesc), C.c_void_p]),
    "bdpt_sky_execute": (C.c_int, [C.c_void_p, C.POINTER(SkyParams), C.POINTER(GBuffer), C.c_void_p, C.c_void_p]),
    "bdpt_bsdf_pdf_query": (C.c_int, [C.c_void_p, C.POINTER(BsdfPdfDesc), C.c_void_p]),
    "bdpt_sky_mis_query": (C.c_int, [C.c_void_p, C.POINTER(SkyMisDesc), C.c_void_p]),
    "bdpt_sky_mis_execute": (C.c_int, [C.c_void_p, C.POINTER(SkyMisParams), C.POINTER(GBuffer), C.c_void_p, C.c_void_p]),
    "bdpt_ris_query": (C.c_int, [C.c_void_p, C.POINTER(RisDesc), C.c_void_p]),
    "bdpt_ris_execute": (C.c_int, [C.c_void_p, C.POINTER(RisParams), C.POINTER(GBuffer), C.c_void_p, C.c_void_p]),
    "bdpt_ris_execute_reservoirs": (C.c_int, [C.c_void_p, C.POINTER(RisParams), C.POINTER(GBuffer), C.c_void_p, C.c_void_p, C.c_void_p]),
    "bdpt_reuse_query": (C.c_int, [C.c_void_p, C.POINTER(ReuseDesc), C.c_void_p]),
    "bdpt_reuse_execute": (C.c_int, [C.c_void_p, C.POINTER(ReuseParams), C.POINTER(GBuffer), C.c_void_p, C.c_void_p]),
    "bdpt_host_env_table": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]),
    "bdpt_host_env_sample": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                        C.c_void_p]),
    "bdpt_host_env_eval": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "bdpt_test_env_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "bdpt_test_host_env_search": (C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "bdpt_host_bvh_refit": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bdpt_host_bvh_refit_pieces": (C.c_int, [C.c_void_p]),
    "bdpt_host_bvh_refit_check": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint32]),
    "bdpt_host_bvh_recs_hash": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "bdpt_host_bvh_refit_info": (C.c_int, [C.c_void_p, C.POINTER(RefitInfo)]),
    "bdpt_ctx_recs_hash": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "bdpt_camera_look_at": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float,
                                      C.c_float, C.c_float, C.c_float, C.POINTER(Camera)]),
    "bdpt_msaa_jitter": (None, [C.c_uint32, C.POINTER(C.c_float)]),
    "bdpt_resize": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, Tile, C.c_uint32]),
    "bdpt_gbuffer_execute": (C.c_int, [C.c_void_p, C.POINTER(GBufferParams), C.POINTER(GBuffer), C.c_void_p]),
    "bdpt_gbuffer_execute_motion": (C.c_int, [C.c_void_p, C.POINTER(GBufferParams), C.POINTER(GBuffer), C.c_void_p, C.c_void_p]),
    "bdpt_execute": (C.c_int, [C.c_void_p, C.POINTER(Params), C.POINTER(GBuffer), C.c_void_p, C.c_void_p]),
    "bdpt_execute_tail": (C.c_int, [C.c_void_p, C.POINTER(Params), C.POINTER(GBuffer), C.c_void_p, C.c_void_p]),
    "bdpt_execute_light_groups": (C.c_int, [C.c_void_p, C.POINTER(Params), C.POINTER(GBuffer), C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "bdpt_execute_grouped": (C.c_int, [C.c_void_p, C.POINTER(Params), C.POINTER(GBuffer), C.c_void_p, C.POINTER(LightGroupDesc),
                                       C.c_void_p]),
    "bdpt_execute_masked": (C.c_int, [C.c_void_p, C.POINTER(Params), C.POINTER(GBuffer), C.c_void_p, C.c_void_p, C.c_void_p]),
    "bdpt_adaptive_reset": (C.c_int, [C.c_void_p, C.POINTER(AdaptiveState), C.c_void_p]),
    "bdpt_adaptive_update": (C.c_int, [C.c_void_p, C.POINTER(AdaptiveParams), C.POINTER(AdaptiveState), C.c_void_p, C.c_void_p]),
    "bdpt_prepare": (C.c_int, [C.c_void_p, C.c_uint32]),
    "bdpt_resize_stripes": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, Stripes, C.c_uint32]),
    "bdpt_stripe_rows": (C.c_uint32, [C.c_uint32, C.c_uint32]),
    "bdpt_get_tile_info": (C.c_int, [C.c_void_p, C.POINTER(TileInfo)]),
    "bdpt_tile_row_ranges": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32]),
    "bdpt_resolve_tile": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bdpt_accumulate_tile": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "bdpt_test_tree_builder": (C.c_int, [C.c_int]),
    "bdpt_bvh_recs_hash": (C.c_int, [C.POINTER(SceneDesc), C.c_int, C.POINTER(C.c_uint64), C.POINTER(BvhInfo)]),
    "bdpt_bvh_build_hash": (C.c_int, [C.POINTER(SceneDesc), C.c_int, C.POINTER(C.c_uint64), C.POINTER(BvhInfo)]),
    "bdpt_splat_buffer": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "bdpt_set_splat_buffer": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "bdpt_resolve": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "bdpt_bmfr_execute": (C.c_int, [C.c_void_p, C.POINTER(BmfrParams), C.POINTER(GBuffer), C.c_void_p, C.c_void_p]),
    "bdpt_bmfr_execute_motion": (C.c_int, [C.c_void_p, C.POINTER(BmfrParams), C.POINTER(GBuffer), C.c_void_p, C.c_void_p, C.c_void_p]),
    "bdpt_bmfr_reset": (C.c_int, [C.c_void_p]),
    "bdpt_bmfr_history_bytes": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "bdpt_bmfr_save_history": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "bdpt_bmfr_load_history": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "bdpt_bmfr_execute_planes": (C.c_int, [C.c_void_p, C.POINTER(BmfrParams), C.POINTER(GBuffer), C.POINTER(BmfrPlanesDesc), C.c_void_p]),
    "bdpt_bmfr_planes_prepare": (C.c_int, [C.c_void_p, C.c_uint32]),
    "bdpt_bmfr_planes_reset": (C.c_int, [C.c_void_p]),
    "bdpt_tile_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "bdpt_tile_unpack": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "bdpt_camera_view_proj": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float,
                                        C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_float)]),
    "bdpt_accumulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64,
                                  C.c_void_p]),
    "bdpt_get_counters": (C.c_int, [C.c_void_p, C.POINTER(Counters)]),
    "bdpt_get_stage_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]),
    "bdpt_enable_stage_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "bdpt_sync": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bdpt_test_rng": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "bdpt_test_trace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]),
    "bdpt_test_trace_shadow": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "bdpt_test_bsdf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "bdpt_get_area_light_info": (C.c_int, [C.c_void_p, C.POINTER(AreaLightInfo)]),
    "bdpt_test_area_light_sample": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "bdpt_test_alpha": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "bdpt_scene_create_cornell": (C.c_void_p, []),
    "bdpt_scene_create_atrium": (C.c_void_p, [C.c_uint32, C.c_uint32]),
    "bdpt_scene_create_atrium_uneven": (C.c_void_p, [C.c_uint32, C.c_uint32]),
    "bdpt_scene_create_courtyard": (C.c_void_p, [C.c_uint32, C.c_uint32, C.c_float]),
    "bdpt_scene_create_soup": (C.c_void_p, [C.c_uint32, C.c_uint32, C.c_float]),
    "bdpt_scene_load": (C.c_void_p, [C.c_char_p, C.c_char_p, C.c_uint32]),
    "bdpt_scene_load_threads": (C.c_int, [C.c_int]),
    "bdpt_scene_destroy": (None, [C.c_void_p]),
    "bdpt_image_load": (C.c_int, [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_void_p, C.c_uint64,
                                  C.c_char_p, C.c_uint32]),
    "bdpt_image_load_hdr": (C.c_int, [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint32]),
    "bdpt_scene_get_desc": (C.c_int, [C.c_void_p, C.POINTER(SceneDesc)]),
    "bdpt_scene_get_camera": (C.c_int, [C.c_void_p, C.c_float, C.POINTER(Camera)]),
}

_lib = None


def load_library(path=None):
    """Load libbdpt_amd.so and bind every prototype.  Raises if anything is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(
            f"{p} not found: the HIP extension is not built (run __graft_entry__.build()). "
            "There is no CPU fallback for the render pass.")
    lib = C.CDLL(p, mode=C.RTLD_GLOBAL)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib
