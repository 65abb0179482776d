"""The walk kernel's sRGB table in LDS and its traversal stack with 28 rows in LDS (kernels.h kWalkStackLds).

walk_kernel copies SceneConst::srgbLut into LDS at entry and shadeHit's texel lookups read it there; the four stack rows
that made room for it live in the context's overflow area (SceneDev::stackOvf), which the any-hit kernel already used.
Both are invisible in the image: every frame here is compared with the CPU oracle bit for bit.
"""
import numpy as np
import pytest

from area_scenes import DescArrays, copy_desc

pytestmark = pytest.mark.gpu


def _flags(model=0, dif=1, spec=1, emis=0, normal=0, alpha=0, double_sided=0):
    return model | (dif << 3) | (spec << 6) | (emis << 9) | (normal << 12) | (alpha << 17) | (double_sided << 19)


def _quad(x, y, z, up):
    (x0, x1), (z0, z1) = x, z
    q = np.array([[x0, y, z0], [x1, y, z0], [x1, y, z1], [x0, y, z1]], np.float32)
    tris = np.array([[0, 2, 1], [0, 3, 2]] if up else [[0, 1, 2], [0, 2, 3]], np.uint32)
    return q, tris


# byte values at both ends of the sRGB curve's linear segment (0 and 10: 10 / 255 <= 0.04045 < 11 / 255), the first of the
# power segment, the middle and the top
EDGE_BYTES = np.array([0, 10, 11, 1, 9, 12, 127, 128, 254, 255], np.uint8)


def _texture(rng, h, w, alpha=None):
    t = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    flat = t.reshape(-1)
    k = min(flat.size, 4 * EDGE_BYTES.size)
    flat[:k] = np.resize(EDGE_BYTES, k)  # every texture starts with the edge values, in every channel
    if alpha is not None:
        t[..., 3] = alpha
    return t


class TexturedBox(DescArrays):
    """The Cornell box with three textured quads in it: a floor cover (metal-rough: sRGB base colour 5 x 3, linear
    roughness / metalness 4 x 4, sRGB emissive 2 x 2, linear RGB normal map 3 x 2), a card floating in the middle
    (alpha-tested, double-sided: sRGB base colour 6 x 5 whose alpha runs over 0, 127, 128 and 255 around the threshold
    0.5) and a cover under the ceiling (specular-glossiness: sRGB 1 x 1 base colour, linear 1 x 1 specular whose alpha is
    the glossiness).  Texture coordinates run from -0.3 to beyond 1, so the wrap column and row of every texture are
    sampled, and the 1 x 1 textures read the spare texel behind them."""

    def __init__(self, pkg, base):
        a = pkg.abi
        c = copy_desc(pkg, base.desc)
        P, N, T, I, M, mats = c["P"], c["N"], c["T"], c["I"], c["M"], c["mats"]
        rng = np.random.default_rng(2026)
        alpha = np.resize(np.array([0, 255, 127, 128, 255, 0, 128, 127, 255], np.uint8), (6 * 5)).reshape(5, 6)
        normal = np.empty((2, 3, 4), np.uint8)
        normal[...] = (128, 128, 255, 255)
        normal[..., :2] += rng.integers(-40, 40, (2, 3, 2)).astype(np.uint8)
        one_srgb = np.array([[[10, 255, 0, 200]]], np.uint8)
        one_lin = np.array([[[255, 0, 11, 128]]], np.uint8)
        textures = [(_texture(rng, 3, 5), True),            # 0 floor base colour, sRGB, neither side a power of two
                    (_texture(rng, 4, 4), False),           # 1 floor roughness / metalness, linear
                    (_texture(rng, 2, 2), True),            # 2 floor emissive, sRGB
                    (normal, False),                        # 3 floor normal map, linear
                    (_texture(rng, 5, 6, alpha), True),     # 4 card base colour + alpha, sRGB
                    (one_srgb, True),                       # 5 ceiling base colour, 1 x 1 sRGB
                    (one_lin, False)]                       # 6 ceiling specular + glossiness, 1 x 1 linear

        def mat(flags, base, spec, emis, norm, threshold=0.5):
            m = a.Material()
            m.baseColor[:] = (0.6, 0.6, 0.6, 1.0)
            m.specular[:] = (0.0, 0.5, 0.0, 0.0)
            m.emissive[:] = (0.0, 0.0, 0.0)
            m.alphaThreshold, m.IoR = threshold, 1.5
            m.texBaseColor, m.texSpecular, m.texEmissive, m.texNormal = base, spec, emis, norm
            m.flags = flags
            mats.append(m)
            return len(mats) - 1

        m_floor = mat(_flags(0, 2, 2, 2, normal=1), 0, 1, 2, 3)
        m_card = mat(_flags(0, 2, 1, 0, alpha=1, double_sided=1), 4, -1, -1, -1)
        m_ceil = mat(_flags(2, 2, 2, 0), 5, 6, -1, -1)
        for (x, z, y, mid, up) in (((30, 520), (30, 520), 2.0, m_floor, True), ((150, 400), (150, 400), 220.0, m_card, True),
                                   ((40, 510), (40, 510), 530.0, m_ceil, False)):
            q, tris = _quad(x, y, z, up)
            v0 = P.shape[0]
            P = np.concatenate([P, q])
            N = np.concatenate([N, np.tile([[0, 1 if up else -1, 0]], (4, 1)).astype(np.float32)])
            T = np.concatenate([T, np.array([[-0.3, -0.3, 0], [2.3, -0.3, 0], [2.3, 1.4, 0], [-0.3, 1.4, 0]], np.float32)])
            I = np.concatenate([I, tris + v0])
            M = np.concatenate([M, np.array([mid, mid], np.uint32)])
        B = np.tile(np.array([[1.0, 0.0, 0.0]], np.float32), (P.shape[0], 1))  # normal-mapped primary hits need bitangents
        super().__init__(a, P, N, T, I, M, mats, textures, c["lights"], B=B)
        self.base = base

    def camera(self, aspect):
        return self.base.camera(aspect)


def _frames_bit_exact(pkg, ob, scene, W, H, depth, frames, channels=True):
    import torch
    pipe = pkg.FramePipeline(scene, W, H, max_depth=depth, mat_index=0)
    seen = 0
    for _ in range(frames):
        gp, p = pipe.render_frame()
        torch.cuda.synchronize()
        orc = ob.OracleRender(pkg.abi, scene.desc, W, H)
        orc.gbuffer(pipe.cam, gp)
        orc.bdpt(pipe.cam, p)
        for ch, on in (("MaterialDiffuse", "materialDiffuse"), ("MaterialSpecRough", "materialSpecRough"), ("Emissive", "emissive"),
                       ("WorldNormal", "worldNormal")) if channels else ():
            g = pipe.channels[ch].float().cpu().numpy().reshape(-1, 4)
            assert np.array_equal(g.view(np.uint32), orc.chan[on].view(np.uint32)), ch
        orc.resolve()
        gpu, ref = pipe.output.cpu().numpy(), orc.image()
        assert np.array_equal(gpu.view(np.uint32), ref.view(np.uint32)), \
            f"{(gpu != ref).any(axis=-1).sum()} pixels differ, max {np.abs(gpu - ref).max()}"
        seen += int((ref[..., :3] > 0).any(axis=-1).sum())
        orc.close()
    pipe.close()
    return seen


def test_textured_frame_bit_exact(pkg, ob):
    """96 x 64, depth 4, GGX: the walk shades hits on sRGB, linear, 1 x 1 and alpha-tested textures from its LDS table."""
    base = pkg.Scene.cornell()
    scene = TexturedBox(pkg, base)
    lit = _frames_bit_exact(pkg, ob, scene, 96, 64, 4, frames=2)
    assert lit > 96 * 64  # most pixels of both frames are lit
    base.close()


def test_walk_stack_beyond_its_lds_rows(pkg, ob):
    """Closest-hit descents that stack more than the walk's 28 LDS rows: the 200 000-triangle soup of large overlapping
    triangles at 64 x 48, depth 4.  Walked on the CPU with the host traversal (scene_bvh.cpp traceHost, which stacks the
    hit children of a node as nodeStep's nearest-first order does) over the 7506 extension rays the oracle traces for
    this frame: the deepest stack is 31 entries (the builder's bound, entries 0-30) and 41 rays stack 29 or more, so
    the frame's walk writes and reads back overflow rows 0-2.  (The same soup at 100 000 triangles stops at 28-29.)"""
    scene = pkg.Scene.soup(99, 200000, 0.9)
    lit = _frames_bit_exact(pkg, ob, scene, 64, 48, 4, frames=1, channels=False)
    assert lit > 0
    scene.close()
