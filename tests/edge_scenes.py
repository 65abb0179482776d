"""Edge-case scenes for the whole BDPT frame (tests/test_edge_scenes_cpu.py, tests/test_gpu_edge_scenes.py): small scenes as
bdpt_scene_desc with a matching camera, in named families that stress what only the frame runs — the gather order, the lazy
rounds, the three NaN rules, the fixed-point splat conversion, occluder hints, MIS prefix products, partial waves and empty
queues.  Seeded, plain numpy; no product code.  At most about 60 triangles each, so that the brute-force scans stay cheap.

Coordinates are small dyadic numbers: a box is [0, 4]^3 moved by a dyadic offset, so that coincidences (a light on a wall, a
wall through the world origin, a light at the camera) are exact in fp32 and in float64 alike.  Every material is
double-sided; the cameras look along +z with tan(fovY / 2) = 1 / 2.

  family               what it is for                                                          control (branch taken)
  ordinary             nothing degenerate                                                      pixelsValid == W * H
  light_on_surface     point lights exactly on a wall's plane, on a shared vertex and within   a valid pixel with |posW - light|^2
                       sqrt(1e-5) of a wall; the camera aims one pixel at the first: getLight- <= 1e-5 (frame 0), light walks traced
                       Data's distance 0 / NaN L, a light walk that starts on geometry
  light_at_camera      the light position bit-equal to the camera position                     equal words; raysNee > 0
  enclosed             the light inside a small closed box: every NEE and connection ray is    own-pixel RGB all +0, alpha == depth on
                       occluded, every pixel with a path goes pending, lazy rounds exhaust     valid pixels (GPU: lazy and hinted rays)
  open                 one floor quad under an open sky, the light above it; with and without  walks shorter than depth: fewer extension
                       ENV_ON_MISS under a constant environment                                rays than valid * steps; invalid pixels
  origin               one box with a window, moved so that the world origin is (a) in open    light walks that end early (zero vertices
                       space, (b) inside a solid block, (c) exactly on a wall                  in pairs); origin/b: the block exists
  black                a checker of all-zero materials beside white ones                       a valid pixel with RGB +0 and alpha 1 in
                                                                                               the connect-only stage
  intensity            three lights drawn from the intensities 0, negative, 1e30, +inf, NaN;   a channel equal to clampUpper in the NEE-only
                       clampUpper 0.9, 1, 0 and the largest value a frame with splats takes    stage (frames of 35 pixels and more)
  specular             GGX roughness at and below the 0.08 clamp, metalness 1, gloss 1, a      all pixels valid; the tests hold the frame
                       mirror-like floor; with and without SPECULAR_FROM_LOBE                  with the flag to differ from the one without
  degenerate_geometry  zero-area triangles, two coplanar duplicate quads, a fan whose shared   the duplicate's pixel shows the lower
                       vertex a pixel centre looks at, -0.0 coordinates, a zero normal         primitive's colour; all pixels valid
  camera               on a wall's plane / inside a solid / looking away / 2^-70 in front of   away: pixelsValid == 0 and no ray at all;
                       a wall: |camera - hit|^2 underflows, under MIS 1 / d^2 overflows        close: the G-buffer's distance is < 1e-6
  valid_counts         caller-made G-buffers over `ordinary` with exactly 0, 1, 63, 64, 65     pixelsValid == k
                       valid pixels at the start, the end and scattered; NaN in invalid pixels
  mis                  ordinary / open / light_on_surface scaled by 2^12 under MIS_POWER and   a channel lit under the uniform weight that
                       MIS_LINEAR: the prefix products underflow, the weight is 0/0            is +0 under MIS, in some stage

Measured on the CPU (`python tests/test_edge_scenes_cpu.py` prints the tables): the oracle (fp32) against the float64 reading
(tests/hlsl_integrator_numpy.py) per family and stage, worst absolute deviation of the own-pixel image and of the splat sums
over the pixels compared (MEASURED).  The asserted bound is bound_of(measured): four times the worst, rounded up to one digit;
`ordinary` must also meet the Cornell cross-check's 2e-5.  LEFT_OUT counts, per case, the pixels whose decision quantity in
the reading lies within MARGIN of a discontinuity (light pick, rintf tie of a splat target, t against tmax, lobe choice); at
most CAP of a case's pixels, which for 1x1 and 7x5 means none.  Class-only families — `mis` (after underflow the fp32 weight
is 0/0 where the float64 one is finite) and `intensity` at the largest legal clampUpper (sums beyond float64's exact integer
range do not arise, but products of 1e30 intensities do leave the fp32 range) — hold alpha words and splat counts only.
"""
import math

import numpy as np

from area_scenes import DescArrays, _light, _quad

FRAMES = ((1, 1), (7, 5), (8, 8), (13, 5), (33, 17))
DEPTHS = (1, 2, 3, 8, 9, 16)
NO_NEE, NO_SPLAT, NO_CONNECT, FROM_LOBE, MIS_POWER, MIS_LINEAR, ENV_ON_MISS = 4, 8, 16, 32, 64, 128, 1024
STAGES = (("plain", 0), ("nee", NO_SPLAT | NO_CONNECT), ("splat", NO_NEE | NO_CONNECT), ("connect", NO_NEE | NO_SPLAT))
JITTER0 = (0.5625, 0.3125)  # the G-buffer pass's pixel jitter of a pipeline's first frame (counter 0xdeadbeef)
FLT_MAX = float(np.finfo(np.float32).max)
CLAMP_LIMIT = 4294967040.0  # 2^32 - 256: the largest clampUpper a frame with splats takes (include/bdpt.h, bdpt_params)
MARGIN = 1e-6
CAP = 0.02
ENV_COLOR = (0.25, 0.5, 0.75, 0.0)
F = np.float32


def bound_of(measured):
    """four times the measured worst deviation, rounded up to one digit"""
    x = 4.0 * measured
    if x == 0:
        return 0.0
    e = np.floor(np.log10(x))
    return float(np.ceil(x / 10 ** e * (1 - 1e-12)) * 10 ** e)


def _mat(a, base, spec=(0.0, 1.0, 0.0, 0.0), model=0):
    m = a.Material()
    m.baseColor[:] = tuple(base) + (1.0,)
    m.specular[:] = spec
    m.emissive[:] = (0.0, 0.0, 0.0)
    m.alphaThreshold, m.IoR = 0.5, 1.5
    m.texBaseColor = m.texSpecular = m.texEmissive = m.texNormal = -1
    m.flags = model | (1 << 3) | (1 << 6) | (1 << 19)  # constant diffuse and specular channels, double-sided
    return m


class Builder:
    """Triangles, one vertex set per face."""

    def __init__(self):
        self.P, self.N, self.I, self.M = [], [], [], []
        self.nv = 0

    def face(self, axis, c, ra, rb, mat, sign=1.0):
        """an axis-aligned quad in the plane x[axis] = c over ra x rb (the other two axes in cyclic order), normal sign * e_axis"""
        q, tris = _quad(ra, c, rb, up=sign > 0)  # columns (a, c, b)
        p = np.zeros_like(q)
        p[:, (axis + 1) % 3], p[:, axis], p[:, (axis + 2) % 3] = q[:, 0], q[:, 1], q[:, 2]
        n = np.zeros((4, 3), np.float32)
        n[:, axis] = sign
        first = len(self.M)
        self.tris(p, tris, n, mat)
        return first

    def tris(self, p, tris, n, mat):
        self.P.append(np.asarray(p, np.float32))
        self.N.append(np.asarray(n, np.float32))
        self.I.append(np.asarray(tris, np.uint32) + self.nv)
        self.M += [mat] * len(tris)
        self.nv += len(p)

    def box(self, lo, hi, mats, inward=True, skip=()):
        """the six faces of [lo, hi]; mats: one material or six (-x, +x, -y, +y, -z, +z); normals point inward or outward"""
        mats = [mats] * 6 if isinstance(mats, int) else list(mats)
        k = 0
        for axis in range(3):
            ra = (lo[(axis + 1) % 3], hi[(axis + 1) % 3])
            rb = (lo[(axis + 2) % 3], hi[(axis + 2) % 3])
            for c, s in ((lo[axis], 1.0), (hi[axis], -1.0)):
                if k not in skip:
                    self.face(axis, c, ra, rb, mats[k], s if inward else -s)
                k += 1

    def arrays(self):
        P, N = np.concatenate(self.P), np.concatenate(self.N)
        return P, N, np.zeros_like(P), np.concatenate(self.I), np.asarray(self.M, np.uint32)


def look(a, pos, aspect, direction=(0.0, 0.0, 1.0), half=0.5, up=None):
    """a camera at pos looking along direction (+-z, or tilted in the y-z plane with a matching `up`): cameraW = direction,
    cameraV = up (default (0, half, 0)), |cameraU| = half * aspect; the three are orthogonal"""
    cam = a.Camera()
    s = 1.0 if direction[2] > 0 else -1.0
    cam.posW[:] = [float(x) for x in pos]
    cam.cameraU[:] = (-s * half * aspect, 0.0, 0.0)
    cam.cameraV[:] = (0.0, half, 0.0) if up is None else up
    cam.cameraW[:] = direction
    return cam


def aimed(a, target, distance, W, H, px, py, aspect):
    """the +z camera whose first-frame G-buffer ray through pixel (px, py) passes through `target`, `distance` in front"""
    cam = look(a, (0, 0, 0), aspect)
    ndx = 2.0 * (px + JITTER0[0]) / W - 1.0
    ndy = -2.0 * (py + JITTER0[1]) / H + 1.0
    d = np.array([cam.cameraU[0] * ndx, cam.cameraV[1] * ndy, 1.0])
    cam.posW[:] = [float(x) for x in np.asarray(target, np.float64) - distance * d]
    return cam


class EdgeFrameScene(DescArrays):
    """A bdpt_scene_desc with the camera of its case: what FramePipeline and OracleRender take."""

    def __init__(self, a, builder, mats, lights, camera):
        P, N, T, I, M = builder.arrays()
        super().__init__(a, P, N, T, I, M, mats, [], lights)
        self._camera = camera

    def camera(self, aspect):
        return self._camera(aspect)

    def close(self):
        pass


WHITE, RED, GREEN, GREY, BLACK = 0, 1, 2, 3, 4


def _palette(a, mat_index):
    """white, red, green, grey, black; matIndex 0 gets GGX parameters of middling roughness"""
    spec = (0.0, 0.5, 0.0, 0.0) if mat_index == 0 else (0.0, 1.0, 0.0, 0.0)
    mats = [_mat(a, c, spec) for c in ((0.75, 0.75, 0.75), (0.625, 0.125, 0.125), (0.125, 0.5, 0.125), (0.5, 0.5, 0.5))]
    mats.append(_mat(a, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0), model=2))  # SpecGloss: diffuse 0, specular 0
    return mats


def _room(b, off=(0.0, 0.0, 0.0), skip=(), block=True):
    lo, hi = np.asarray(off, np.float32), np.asarray(off, np.float32) + 4
    b.box(lo, hi, (RED, GREEN, WHITE, WHITE, GREY, WHITE), skip=skip)
    if block:  # on the floor
        b.box(lo + np.array([2.5, 0, 2], np.float32), lo + np.array([3.5, 1, 3], np.float32), GREY, inward=False)


def _point(a, pos, inten=(8.0, 8.0, 8.0)):
    return _light(a, a.LIGHT_POINT, pos, (0.0, -1.0, 0.0), inten)


def _cam_room(a, off=(0.0, 0.0, 0.0)):
    return lambda aspect: look(a, (off[0] + 2.0, off[1] + 2.0, off[2] + 0.25), aspect)


class Case:
    def __init__(self, family, variant, W, H, depth, mat, flags=0, clamp=0.9, min_t=None, valid=None, env=False, class_only=False):
        self.family, self.variant, self.W, self.H, self.depth, self.mat = family, variant, W, H, depth, mat
        # gMinT = 2^-10 in a 4-unit room (the default 1e-4 is below what fp32 knows of a hit point there); `mis` scales with its scene
        self.min_t = (4.0 if family == "mis" else 2.0 ** -10) if min_t is None else min_t
        self.flags, self.clamp, self.valid, self.env, self.class_only = flags, clamp, valid, env, class_only

    @property
    def id(self):
        v = f"/{self.variant}" if self.variant else ""
        f = f" f{self.flags}" if self.flags else ""
        c = f" c{self.clamp:g}" if self.clamp != 0.9 else ""
        return f"{self.family}{v} {self.W}x{self.H} d{self.depth} m{self.mat}{f}{c}"

    def scene(self, a):
        return build_scene(a, self)


def build_scene(a, case):
    """the EdgeFrameScene of a case; case.W / case.H matter only to cameras that aim a pixel"""
    fam, var, W, H = case.family, case.variant, case.W, case.H
    b = Builder()
    mats = _palette(a, case.mat)
    cam = _cam_room(a)
    lights = [_point(a, (2.0, 3.5, 2.0))]
    if fam in ("ordinary", "valid_counts") or (fam == "mis" and var.startswith("ordinary")):
        _room(b)
        lights.append(_point(a, (1.0, 2.0, 3.0), (2.0, 3.0, 4.0)))
    elif fam == "light_on_surface" or (fam == "mis" and var.startswith("light_on_surface")):
        _room(b)
        # on the back wall's plane (z = 4), on the corner shared by three faces, and 2^-9 < sqrt(1e-5) off the left wall
        lights = [_point(a, (1.5, 2.5, 4.0)), _point(a, (4.0, 4.0, 4.0), (4.0, 4.0, 4.0)), _point(a, (2.0 ** -9, 1.0, 2.0), (2.0, 4.0, 2.0))]
        px, py = W // 2, H // 2
        cam = lambda aspect: aimed(a, (1.5, 2.5, 4.0), 3.5, W, H, px, py, aspect)  # noqa: E731
    elif fam == "light_at_camera":
        _room(b)
        lights = [_point(a, (2.0, 2.0, 0.25))]
    elif fam == "enclosed":
        _room(b, block=False)
        # three shells: a connection from an eye vertex ON the outer shell (its start is skipped by minT) to a light vertex ON
        # the inner one (an end-point tie) still crosses the middle one
        for lo, hi in (((1.75, 3.25, 1.75), (2.25, 3.75, 2.25)), ((1.625, 3.125, 1.625), (2.375, 3.8125, 2.375)), ((1.5, 3.0, 1.5), (2.5, 3.875, 2.5))):
            b.box(np.array(lo, np.float32), np.array(hi, np.float32), WHITE)
    elif fam == "open" or (fam == "mis" and var.startswith("open")):
        b.face(1, 0.0, (0.0, 8.0), (-4.0, 4.0), WHITE, 1.0)  # (z range, x range)
        lights = [_point(a, (0.0, 2.0, 4.0))]
        cam = lambda aspect: look(a, (0.0, 1.0, 0.0), aspect, (0.0, -0.5, 1.0), up=(0.0, 0.5, 0.25))  # noqa: E731
    elif fam == "origin":
        # the room's far ceiling half is a window: walks leave, and the vertices past a walk's end are the zero vertex
        off = {"a": (-2.0, -2.0, -1.0), "b": (-3.0, -0.5, -2.5), "c": (0.0, -2.0, -1.0)}[var]
        lo = np.asarray(off, np.float32)
        b.box(lo, lo + 4, (RED, GREEN, WHITE, WHITE, GREY, WHITE), skip=(3,))
        b.face(1, float(lo[1] + 4), (float(lo[2]), float(lo[2] + 2)), (float(lo[0]), float(lo[0] + 4)), WHITE, -1.0)
        b.box(lo + np.array([2.5, 0, 2], np.float32), lo + np.array([3.5, 1, 3], np.float32), GREY, inward=False)
        cam = _cam_room(a, off)
        lights = [_point(a, (off[0] + 2.0, off[1] + 3.5, off[2] + 2.0))]
    elif fam == "black":
        lo = np.zeros(3, np.float32)
        b.box(lo, lo + 4, (RED, GREEN, WHITE, WHITE, GREY, WHITE), skip=(2, 5))
        for i in range(4):  # floor (y = 0) and back wall (z = 4) as 4 x 4 checkers of black and white
            for j in range(4):
                m = BLACK if (i + j) % 2 else WHITE
                b.face(1, 0.0, (float(j), j + 1.0), (float(i), i + 1.0), m, 1.0)  # ranges: (z, x)
        for i in range(2):
            for j in range(2):
                b.face(2, 4.0, (2.0 * i, 2.0 * i + 2), (2.0 * j, 2.0 * j + 2), BLACK if (i + j) % 2 else WHITE, -1.0)
    elif fam == "intensity":
        _room(b)
        table = {"0": 0.0, "neg": -4.0, "big": 1e30, "inf": math.inf, "nan": math.nan}
        pos = ((1.75, 3.5, 1.75), (1.0, 2.0, 3.25), (3.0, 3.0, 1.0))  # in no face's plane: NdotL == 0 times +inf would be a tie
        # the third channel stays finite: a term of a NaN light is (NaN, NaN, x), which tells the NaN rules apart
        lights = [_point(a, p, (table[k], 0.5 * table[k] if k != "0" else 4.0, 2.0 + n)) for n, (p, k) in enumerate(zip(pos, var.split("_")))]
    elif fam == "specular":
        lo = np.zeros(3, np.float32)
        # MetalRough: specular = (-, linear roughness, metalness, -); SpecGloss (model 2): (F0 rgb, gloss)
        mats += [_mat(a, (0.75, 0.75, 0.75), (0.0, 0.08, 1.0, 0.0)), _mat(a, (0.75, 0.5, 0.25), (0.0, 0.0625, 0.5, 0.0)),
                 _mat(a, (0.5, 0.5, 0.5), (0.0, 0.0, 1.0, 0.0)), _mat(a, (0.25, 0.25, 0.25), (0.75, 0.75, 0.75, 1.0), model=2)]
        b.box(lo, lo + 4, (6, 7, 5, WHITE, 8, 6))  # floor (-y): roughness at the clamp, metalness 1: mirror-like
    elif fam == "degenerate_geometry":
        _room(b)
        z = F(-0.0)
        # two coplanar duplicate quads in front of the back wall, red (lower primitives) then green
        b.face(2, 3.5, (0.5, 1.5), (2.0, 3.0), RED, -1.0)
        b.face(2, 3.5, (0.5, 1.5), (2.0, 3.0), GREEN, -1.0)
        # zero-area triangles: a repeated corner, three collinear corners
        n = np.tile(np.array([[0, 0, -1]], np.float32), (3, 1))
        b.tris([[1, 1, 3], [1, 1, 3], [2, 1, 3]], [[0, 1, 2]], n, WHITE)
        b.tris([[1, 1, 3], [2, 2, 3], [3, 3, 3]], [[0, 1, 2]], n, WHITE)
        # a fan of eight triangles around (2, 2, 3): the camera (2, 2, 0.25) aims a pixel centre at the shared vertex
        ang = [k * math.pi / 4 for k in range(9)]
        ring = [[2 + 0.5 * math.cos(t), 2 + 0.5 * math.sin(t), 3.0] for t in ang]
        for k in range(8):
            nn = np.tile(np.array([[0, 0, -1]], np.float32), (3, 1))
            if k == 3:
                nn[0] = 0.0  # a vertex normal of zero length (at the ring, not at the hub)
            b.tris([ring[k], ring[k + 1], [2, 2, 3]], [[0, 1, 2]], nn, WHITE if k % 2 else GREY)
        # a quad with -0.0 coordinates on the floor's plane corner
        b.tris([[z, 0.5, z], [1, 0.5, z], [1, 0.5, 1], [z, 0.5, 1]], [[0, 2, 1], [0, 3, 2]], np.tile(np.array([[z, 1, z]], np.float32), (4, 1)), GREEN)
        px, py = W // 2, H // 2
        cam = lambda aspect: aimed(a, (2.0, 2.0, 3.0), 2.75, W, H, px, py, aspect)  # noqa: E731
    elif fam == "camera":
        _room(b)
        pos, d = {"on_wall": ((2.0, 2.0, 0.0), (0.0, 0.0, 1.0)), "in_solid": ((3.0, 0.5, 2.5), (0.0, 0.0, 1.0)),
                  "away": ((2.0, 2.0, -1.0), (0.0, 0.0, -1.0)), "close": ((2.0, 2.0, 2.0 ** -70), (0.0, 0.0, -1.0))}[var]
        cam = lambda aspect: look(a, pos, aspect, d)  # noqa: E731
    else:
        raise KeyError(fam)
    scale = 2.0 ** 12 if fam == "mis" else 1.0
    sc = EdgeFrameScene(a, b, mats, lights, cam)
    if scale != 1.0:
        sc.P *= F(scale)
        for l in sc.lights:
            for k in range(3):
                l.posW[k] *= scale
                l.intensity[k] *= scale * scale
        inner = sc._camera

        def scaled(aspect):
            c = inner(aspect)
            for k in range(3):
                c.posW[k] *= scale
            return c
        sc._camera = scaled
    return sc


INTENSITY_SETS = ("0_neg_big", "inf_nan_0", "big_inf_neg", "nan_0_inf", "neg_nan_big")
CLAMPS = (0.9, 1.0, 0.0, CLAMP_LIMIT)


def cases():
    """every case, as the issue's matrix: each family at depth 3 on all frames; depths 1, 2, 8, 9, 16 on one or two frames
    for origin, open, black and mis; both material models; SPECULAR_FROM_LOBE for `specular`"""
    out = []
    k = 0

    def add(family, variant="", **kw):
        nonlocal k
        for W, H in kw.pop("frames", FRAMES):
            out.append(Case(family, variant, W, H, kw.get("depth", 3), kw.get("mat", k % 2), kw.get("flags", 0), kw.get("clamp", 0.9),
                            env=kw.get("env", False), class_only=kw.get("class_only", False), valid=kw.get("valid")))
            k += 1

    add("ordinary")
    add("light_on_surface")
    add("light_at_camera")
    add("enclosed")
    add("open")
    add("open", flags=ENV_ON_MISS, env=True)
    for v in "abc":
        add("origin", v)
    add("black")
    for n, v in enumerate(INTENSITY_SETS):
        add("intensity", v, clamp=CLAMPS[n % 4], class_only=CLAMPS[n % 4] == CLAMP_LIMIT)
    for c in CLAMPS[1:]:
        add("intensity", INTENSITY_SETS[1], clamp=c, frames=((13, 5),), class_only=c == CLAMP_LIMIT)
    add("specular", mat=0)
    add("specular", mat=0, flags=FROM_LOBE)
    add("specular", mat=1, frames=((8, 8),))
    add("degenerate_geometry")
    for v in ("on_wall", "in_solid", "away", "close"):
        add("camera", v)
    for name, (W, H, idx) in valid_sets().items():
        out.append(Case("valid_counts", name, W, H, 3, k % 2, valid=idx))
        k += 1
    add("camera", "close", flags=MIS_POWER, class_only=True, frames=((7, 5),))
    for v in ("ordinary", "open", "light_on_surface"):
        add("mis", v + "/power", flags=MIS_POWER, class_only=True)
        add("mis", v + "/linear", flags=MIS_LINEAR, class_only=True, frames=((7, 5), (13, 5)))
    for d in (1, 2, 8, 9, 16):
        fr = ((13, 5),) if d >= 9 else ((7, 5), (13, 5))
        add("origin", "b", depth=d, frames=fr)
        add("origin", "a" if d % 2 else "c", depth=d, frames=fr[:1])
        add("open", depth=d, frames=fr)
        add("black", depth=d, frames=fr)
        add("mis", "ordinary/power", depth=d, flags=MIS_POWER, class_only=True, frames=((7, 5),))
        add("mis", "open/linear", depth=d, flags=MIS_LINEAR, class_only=True, frames=((7, 5),))
    return out


def valid_sets():
    """name -> (W, H, indices of the valid pixels): exactly 0, 1, 63, 64, 65 valid pixels at the start, the end, scattered"""
    rng = np.random.default_rng(20261021)
    out = {}
    for W, H in ((13, 5), (33, 17)):
        n = W * H
        for k in (0, 1, 63, 64, 65):
            if k > n:
                continue
            places = {"start": np.arange(k), "end": np.arange(n - k, n), "scattered": np.sort(rng.choice(n, k, replace=False))}
            for where, idx in places.items():
                if k == 0 and where != "start":
                    continue
                if (W, H) == (33, 17) and where != "scattered" and k not in (0, 64):
                    continue
                out[f"{k}_{where}_{W}x{H}"] = (W, H, idx.astype(np.int64))
    return out


def mask_gbuffer(chan, W, H, idx):
    """the caller-made G-buffer of a valid_counts case, in place: pixels outside idx lose their geometry (worldPosition.w = 0)
    and every second one of them gets NaN in its other channels; chan: name -> (W * H, 4) float32"""
    keep = np.zeros(W * H, bool)
    keep[idx] = True
    gone = np.nonzero(~keep)[0]
    chan["worldPosition"][gone, 3] = 0.0
    for name in ("worldNormal", "materialSpecRough", "materialExtra", "emissive"):
        chan[name][gone[::2]] = np.nan
    chan["worldPosition"][gone[::2], :3] = np.nan
    chan["materialDiffuse"][gone[1::4]] = np.nan  # (the background colour the pass copies through)


def control(case, cnt, chan, own, stage_images, uniform=None):
    """The positive control of a case's family on oracle results -> (holds, what was seen).  cnt: counters of the plain frame
    as a dict; chan: the G-buffer channels; own: the plain frame's own-pixel image (n, 4) before the splat fold-in;
    stage_images: stage name -> own-pixel image (n, 4), `splat` -> (splat words (n, 4) uint64); uniform: the same of the frame
    without the MIS flags (mis only)."""
    fam, var, n, D = case.family, case.variant, case.W * case.H, case.depth
    valid = chan["worldPosition"][:, 3] != 0
    nv = int(valid.sum())
    if fam == "ordinary":
        return cnt["pixelsValid"] == n, cnt["pixelsValid"]
    if fam == "valid_counts":
        return cnt["pixelsValid"] == len(case.valid) == nv, (cnt["pixelsValid"], len(case.valid))
    if fam == "light_on_surface":
        d2 = ((chan["worldPosition"][valid, :3].astype(np.float64) - np.array([1.5, 2.5, 4.0])) ** 2).sum(axis=1)
        return d2.min() <= 1e-5 and cnt["raysLightExtend"] > 0, (float(d2.min()), cnt["raysLightExtend"])
    if fam == "light_at_camera":
        return cnt["raysNee"] > 0 and nv == n, cnt["raysNee"]
    if fam == "enclosed":
        rgb = stage_images["nee"][valid, :3].view(np.uint32), stage_images["connect"][valid, :3].view(np.uint32)
        alpha_ok = (stage_images["nee"][valid, 3] == D).all() and (stage_images["connect"][valid, 3] == 0).all()
        return nv == n and not rgb[0].any() and not rgb[1].any() and alpha_ok, (nv, int(rgb[0].any()), int(rgb[1].any()), bool(alpha_ok))
    if fam == "open":
        short = D < 2 or (cnt["raysLightExtend"] < nv * D and (D < 3 or cnt["raysEyeExtend"] < nv * (D - 1)))
        return nv > 0 and short and (n == 1 or nv < n), (nv, cnt["raysLightExtend"], cnt["raysEyeExtend"])
    if fam == "origin":
        return nv == n and (n < 30 or D < 2 or cnt["raysLightExtend"] < nv * D), (nv, cnt["raysLightExtend"])
    if fam == "black":
        if D < 2:
            return nv == n, nv
        c = stage_images["connect"]
        hit = valid & (c[:, 3] == 1) & ~c[:, :3].view(np.uint32).any(axis=1)
        return n < 30 or hit.any(), int(hit.sum())
    if fam == "intensity":
        nee = stage_images["nee"][valid, :3]
        top = (nee == F(case.clamp)).any() if case.clamp > 0 else not nee.view(np.uint32).any()
        return n < 30 or bool(top), float(np.nanmax(nee)) if nee.size else None
    if fam == "specular":
        return nv == n, nv
    if fam == "degenerate_geometry":
        # the pixel that sees the duplicate quads' centre (1, 2.5, 3.5) shows red, the lower primitive
        dif = chan["materialDiffuse"]
        p = chan["worldPosition"]
        on_dup = valid & (np.abs(p[:, 2] - 3.5) < 1e-3)
        red = np.allclose(dif[on_dup, :3], (0.625, 0.125, 0.125), atol=1e-3) if on_dup.any() else True
        return nv == n and red and (n < 30 or on_dup.any()), (nv, int(on_dup.sum()))
    if fam == "camera":
        if var == "away":
            rays = sum(cnt[k] for k in ("raysEyeExtend", "raysLightExtend", "raysNee", "raysSplat", "raysConnect"))
            return nv == 0 and cnt["pixelsValid"] == 0 and rays == 0, (nv, rays)
        if var == "close":
            return nv == n and (chan["worldNormal"][:, 3] < 1e-6).all(), nv
        return nv == n, nv
    if fam == "mis":
        lost = 0
        for st in ("nee", "splat", "connect"):
            u, m = uniform[st][:, :3], stage_images[st][:, :3]
            lost += int(((u > 0) & (m == 0)).sum())
        return nv > 0 and (n == 1 or lost > 0), (nv, lost)
    raise KeyError(fam)


# family/stage -> worst |oracle - float64 reading| over the pixels compared (own-pixel image, splat sums), measured; stages: nee,
# splat, connect (ORACLE_CONNECT_ALL_VISIBLE), connect_traced.  `specular/nee` is large because the GGX lobe at the roughness
# clamp (alpha = 0.0064) has D up to 1 / (pi alpha^2) = 7.8e3: a relative 1e-7 of the half vector is 1e-4 of the term before
# the clamp.  `mis` and the largest-clampUpper cases are class-only and have no entry.
MEASURED = {
    "ordinary/nee": 5.7e-06,
    "ordinary/splat": 5.5e-08,
    "ordinary/connect": 2.5e-07,
    "light_on_surface/nee": 4.0e-06,
    "light_on_surface/splat": 2.7e-07,
    "light_on_surface/connect": 9.4e-07,
    "light_at_camera/nee": 4.9e-06,
    "light_at_camera/splat": 1.8e-07,
    "light_at_camera/connect": 3.8e-07,
    "enclosed/nee": 0.0e+00,
    "enclosed/splat": 0.0e+00,
    "enclosed/connect": 3.5e-06,
    "enclosed/connect_traced": 0.0e+00,
    "open/nee": 2.2e-07,
    "open/splat": 2.3e-07,
    "open/connect": 2.3e-07,
    "open/connect_traced": 2.3e-07,
    "origin/nee": 6.3e-06,
    "origin/splat": 1.7e-07,
    "origin/connect": 1.4e-05,
    "black/nee": 1.1e-06,
    "black/splat": 7.6e-08,
    "black/connect": 1.2e-05,
    "intensity/nee": 3.7e-06,
    "intensity/splat": 4.5e-08,
    "intensity/connect": 2.6e-07,
    "specular/nee": 2.9e-04,
    "specular/splat": 9.0e-06,
    "specular/connect": 1.3e-06,
    "degenerate_geometry/nee": 6.9e-07,
    "degenerate_geometry/splat": 9.5e-08,
    "degenerate_geometry/connect": 7.8e-07,
    "camera/nee": 1.3e-06,
    "camera/splat": 1.7e-06,
    "camera/connect": 1.1e-06,
    "valid_counts/nee": 5.7e-06,
    "valid_counts/splat": 7.2e-08,
    "valid_counts/connect": 5.8e-07,
}

# case id -> pixels left out (decision margins), of W * H; a case without an entry leaves none out.  With the oracle's scan
# as the reading's tracer and the all-visible hooks on the tie families, no case of this matrix leaves a pixel out.
LEFT_OUT = {}


# ---- the oracle over a case (oracle/liboracle.so through tests/oracle_binding.py), as FramePipeline drives a frame ----------
def frame_params(pkg, case, frame, stage_flags=0):
    """(bdpt_gbuffer_params, bdpt_params) of a FramePipeline's frame number `frame` for the case"""
    A = pkg.abi
    gp = A.GBufferParams()
    count = 0xdeadbeef + frame
    gp.pixelJitter[0], gp.pixelJitter[1] = pkg.msaa_jitter(count)
    gp.frameCount, gp.useThinLens, gp.focalLen, gp.lensRadius = count & 0xFFFFFFFF, 0, 1.0, 1.0 / 64.0
    gp.envWidth = gp.envHeight = 128
    for i, c in enumerate((0.5, 0.5, 0.8, 1.0)):
        gp.envColor[i] = c
    p = A.Params()
    p.minT, p.frameCount, p.matIndex, p.maxDepth = case.min_t, (0x1337 + frame) & 0xFFFFFFFF, case.mat, case.depth
    p.refractiveIndex, p.emitMult, p.clampUpper, p.flags = 1.0, 1.0, case.clamp, case.flags | stage_flags
    p.pixelJitter[0], p.pixelJitter[1] = pkg.msaa_jitter(0x1337 + frame)
    return gp, p


class OracleResult:
    """One oracle frame: G-buffer channels, own-pixel image, splat words, counters; resolved() folds the splats in."""

    def __init__(self, orc, cnt):
        self.chan = {k: v.copy() for k, v in orc.chan.items() if k != "out"}
        self.own, self.splat = orc.chan["out"].copy(), orc.splat.copy()
        self.cnt = {n: int(getattr(cnt, n)) for n, _ in cnt._fields_}
        orc.resolve()
        self.image = orc.chan["out"].copy()


def oracle_case(pkg, ob, case, frames=(0,), stages=STAGES, oflags=None, drop_flags=0):
    """(frame, stage name) -> OracleResult with the brute-force scan (oflags: other ORACLE_* flags; drop_flags: BDPT_PARAM_* to
    clear, for the uniform-weight frame of a mis case)"""
    A = pkg.abi
    sc = case.scene(A)
    cam = sc.camera(case.W / case.H)
    orc = ob.OracleRender(A, sc.desc, case.W, case.H)
    if case.env:
        orc.set_environment(color=ENV_COLOR)
    flags = ob.ORACLE_BRUTE_FORCE if oflags is None else oflags
    out = {}
    for frame in frames:
        for name, fl in stages:
            gp, p = frame_params(pkg, case, frame, fl)
            p.flags &= ~drop_flags
            orc.gbuffer(cam, gp, flags=flags)
            if case.valid is not None:
                mask_gbuffer(orc.chan, case.W, case.H, case.valid)
            out[frame, name] = OracleResult(orc, orc.bdpt(cam, p, flags=flags))
    orc.close()
    return out


def control_of(pkg, ob, case, results=None):
    """control() of the case on frame 0 of the oracle"""
    r = results if results is not None and all((0, s) in results for s, _ in STAGES) else oracle_case(pkg, ob, case)
    images = {s: r[0, s].own for s, _ in STAGES}
    images["splat"] = r[0, "splat"].splat
    uniform = None
    if case.family == "mis":
        u = oracle_case(pkg, ob, case, drop_flags=MIS_POWER | MIS_LINEAR)
        uniform = {s: u[0, s].own for s, _ in STAGES}
        uniform["splat"] = u[0, "splat"].splat
    return control(case, r[0, "plain"].cnt, r[0, "plain"].chan, r[0, "plain"].own, images, uniform)
