"""Layout of the path-vertex record and of the triangle shading record (kernels.hip "Path vertices", kernels.h kShadeRecF4).

The walk's shading pass reads throughput, RNG state and ray origin of vertex k: q0 and q1 of its 96-byte record, which must
share one 128-byte line for every pixel, and one 128-byte shading record, which must not straddle two.  The CPU tests restate
the field map and do the line arithmetic; the GPU tests compare frames with the CPU oracle bit for bit on every path that
reads or writes a record: the walk at depths where it never extends, first uses a copied seed and runs long, sub-paths that
miss (ghost vertices) with and without the environment / emissive terms, the masked and light-group instances, the 16-lane
generators and the MIS prefix products.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from area_scenes import EMISSIVE_HITS, ENV_ON_MISS, MIS_POWER, DescArrays

LINE = 128
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fyp-bidirectionalpathtracer_amd", "csrc")

# field -> (float4 slot, first component, components); the record before this layout and now
OLD = {"pos": (0, 0, 3), "rough": (0, 3, 1), "N": (1, 0, 3), "isSpec": (1, 3, 1), "dif": (2, 0, 3), "pdf": (2, 3, 1),
       "spec": (3, 0, 3), "color": (4, 0, 3), "V": (5, 0, 3)}
NEW = {"color": (0, 0, 3), "seed": (0, 3, 1), "pos": (1, 0, 3), "rough": (1, 3, 1), "N": (2, 0, 3), "isSpec": (2, 3, 1),
       "dif": (3, 0, 3), "pdf": (3, 3, 1), "spec": (4, 0, 3), "V": (5, 0, 3)}


def _constant(name):
    text = open(os.path.join(_CSRC, "kernels.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def _floats(layout):
    """field -> the float offsets it occupies within the record"""
    return {f: [q * 4 + c + i for i in range(n)] for f, (q, c, n) in layout.items()}


def test_field_map_is_the_old_fields_plus_the_seed():
    nf4 = _constant("NF4")
    assert nf4 == 6  # 96 bytes, as before
    old, new = _floats(OLD), _floats(NEW)
    assert set(new) == set(old) | {"seed"}
    for f in old:
        assert len(new[f]) == len(old[f]), f  # every field keeps its width
    used = sorted(x for v in new.values() for x in v)
    assert len(used) == len(set(used)) and used[-1] < nf4 * 4  # no two fields share a float, none leaves the record
    # the seed took one of the three floats that were padding (the colour's spare word, then q4.w, now q0.w)
    spare_old = set(range(nf4 * 4)) - {x for v in old.values() for x in v}
    assert len(spare_old) == 3 and len(set(range(nf4 * 4)) - set(used)) == 2
    # what the walk's shading pass reads of vertex k sits in q0, q1; the four float4 a generator reads are q1..q4
    assert {NEW[f][0] for f in ("color", "seed")} == {0} and {NEW[f][0] for f in ("pos", "rough")} == {1}
    assert [NEW[f][0] for f in ("pos", "N", "dif", "spec")] == [1, 2, 3, 4]
    # fieldQ / ldPlane1 of kernels.hip state the same map
    text = open(os.path.join(_CSRC, "kernels.hip")).read()
    m = re.search(r"fieldQ\(int f\) \{ return (.*?); \}", text).group(1)
    assert m == "f == F_COL ? 0 : f == F_POS ? 1 : f == F_N ? 2 : f == F_DIF ? 3 : f == F_SPEC ? 4 : 5"
    assert "(f == F_ROUGH) ? 1 : (f == F_ISSPEC ? 2 : 3)" in text


def test_walk_reads_of_a_vertex_stay_in_one_line():
    stride = _constant("NF4") * 16
    for p in range(1024):  # records of one (path, k) plane; a plane starts at a multiple of 96 * Np bytes from a 128-byte-aligned base
        first, last = stride * p, stride * p + 31
        assert first // LINE == last // LINE, p
    # the plane bases themselves: any multiple of the stride keeps bytes 0..31 of every record inside a line
    for np_ in (1, 3, 64, 2047, 96 * 64, 1920 * 1080):
        assert (stride * np_) % 32 == 0
    # (the old places, q0 and q4 of a record, shared a line for two of the four residues of 96 p mod 128 only)
    same = sum((stride * p) // LINE == (stride * p + 64 + 15) // LINE for p in range(1024))
    assert same == 512


def test_shading_record_is_one_line():
    rec = _constant("kShadeRecF4") * 16
    assert rec == LINE
    for t in range(1024):
        assert (rec * t) // LINE == (rec * t + rec - 1) // LINE


# ---- GPU: frames against the oracle, bit for bit ----------------------------------------------------------------------
ENV = (0.3, 0.45, 0.7, 1.0)
SENTINEL = 7.0  # (a value no frame writes)


class OpenBox(DescArrays):
    """The textured Cornell box without its ceiling and the cover under it (the box has no front wall: the camera looks in
    through it), so eye and light sub-paths leave the scene at every bounce and end in ghost vertices."""

    def __init__(self, pkg, tb):
        n = tb.I.shape[0]
        keep = np.ones(n, bool)
        keep[[2, 3, n - 2, n - 1]] = False  # ceiling (second quad of the box), ceiling cover (last quad added)
        assert (tb.P[tb.I[~keep]][..., 1] > 500).all()
        super().__init__(pkg.abi, tb.P, tb.N, tb.T, tb.I[keep], tb.M[keep], list(tb.mats), tb.textures, list(tb.lights), B=tb.B)
        self.base = tb.base

    def camera(self, aspect):
        return self.base.camera(aspect)


@pytest.fixture(scope="module")
def boxes(pkg):
    import test_gpu_walk_lds_tables as lds
    base = pkg.Scene.cornell()
    tb = lds.TexturedBox(pkg, base)
    yield {"box": tb, "open": OpenBox(pkg, tb)}
    base.close()


_refs = {}


def _oracle(pkg, ob, scene, name, pipe, gp, p, env):
    """The oracle's image of the frame (gp, p): computed once per frame description, shared, never written to."""
    key = (name, pipe.W, pipe.H, int(p.maxDepth), int(p.flags), int(p.matIndex), int(p.frameCount), env)
    if key not in _refs:
        orc = ob.OracleRender(pkg.abi, scene.desc, pipe.W, pipe.H)
        if env:
            orc.set_environment(None, ENV)
        orc.gbuffer(pipe.cam, gp)
        orc.bdpt(pipe.cam, p)
        orc.resolve()
        ref = orc.image().copy()
        ref.setflags(write=False)
        orc.close()
        _refs[key] = ref
    return _refs[key]


def _same(gpu, ref, label):
    gpu = np.ascontiguousarray(gpu, np.float32)
    assert np.array_equal(gpu.view(np.uint32), ref.view(np.uint32)), \
        f"{label}: {(gpu != ref).any(axis=-1).sum()} pixels differ, max {np.abs(gpu - ref).max()}"


def _plain(pkg, ob, boxes, name, W, H, depth, flags=0, mat=0):
    import torch
    scene = boxes[name]
    pipe = pkg.FramePipeline(scene, W, H, max_depth=depth, mat_index=mat)
    env = bool(flags & ENV_ON_MISS)
    if env:
        pipe.ctx.set_environment(None, 0, 0, ENV)
    gp, p = pipe.render_frame(extra_flags=flags)
    torch.cuda.synchronize()
    gpu = pipe.output.cpu().numpy().copy()
    cnt = pipe.ctx.counters().as_dict()
    ref = _oracle(pkg, ob, scene, name, pipe, gp, p, env)
    pipe.close()
    _same(gpu, ref, f"{name} {W}x{H} depth {depth} flags {flags}")
    assert (ref[..., :3] > 0).any(axis=-1).sum() > W * H // 4  # the frame is not empty
    return gpu, cnt


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2, 3, 8])
def test_textured_box_depths(pkg, ob, boxes, depth):
    """96 x 64, GGX.  Depth 1: the eye walk never extends (only light vertex 0's seed is read); depth 2: the first frame in
    which a seed the walk copied into vertex k + 1 is drawn from; depth 8: the bench's."""
    _, cnt = _plain(pkg, ob, boxes, "box", 96, 64, depth)
    assert (cnt["raysEyeExtend"] > 0) == (depth >= 2) and cnt["raysLightExtend"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, ENV_ON_MISS | EMISSIVE_HITS], ids=["plain", "ext"])
def test_open_box_ghost_vertices(pkg, ob, boxes, flags):
    """The open box at 96 x 64, depth 6: sub-paths miss at several bounces.  Plain, and the EXT instance of the walk, whose
    environment term on a miss multiplies the throughput read from q0."""
    D = 6
    gpu, cnt = _plain(pkg, ob, boxes, "open", 96, 64, D, flags)
    # fewer extension rays than sub-paths that never miss would trace: ghost vertices were stored on both sides
    assert 0 < cnt["raysEyeExtend"] < cnt["pixelsValid"] * (D - 1)
    assert 0 < cnt["raysLightExtend"] < cnt["pixelsValid"] * D
    if flags:
        dark, _ = _plain(pkg, ob, boxes, "open", 96, 64, D, 0)
        assert gpu[..., :3].sum() > dark[..., :3].sum()  # the environment adds light


def _frame(pkg, boxes, W, H, depth, flags=0):
    import torch
    pipe = pkg.FramePipeline(boxes["box"], W, H, max_depth=depth, mat_index=0)
    gp = pipe.gbuffer_params()
    pipe.ctx.gbuffer_execute(gp, pipe.gb, pipe._stream_ptr())
    p = pipe.bdpt_params(flags)
    torch.cuda.synchronize()
    return pipe, gp, p


@pytest.mark.gpu
def test_masked_frame(pkg, ob, boxes):
    """bdpt_execute_masked (the MASKED walk instance) on the box at 96 x 64, depth 3: active pixels the oracle's bits."""
    import torch
    pipe, gp, p = _frame(pkg, boxes, 96, 64, 3)
    rng = np.random.default_rng(5)
    mask = np.kron(rng.random((16, 24)) < 0.5, np.ones((4, 4), bool))[:64, :96].astype(np.uint8)
    m = torch.as_tensor(mask, device=pipe.dev)
    out = torch.full((64, 96, 4), SENTINEL, dtype=torch.float32, device=pipe.dev)
    pipe.ctx.execute_masked(p, pipe.gb, C.c_void_p(m.data_ptr()), C.c_void_p(out.data_ptr()), pipe._stream_ptr())
    torch.cuda.synchronize()
    ref = _oracle(pkg, ob, boxes["box"], "box", pipe, gp, p, False)
    o, act = out.cpu().numpy(), mask != 0
    pipe.close()
    assert act.any() and (~act).any()
    _same(o[act], ref[act], "masked, active pixels")
    assert (o[~act] == SENTINEL).all()


@pytest.mark.gpu
def test_light_groups_frame(pkg, ob, boxes):
    """bdpt_execute_light_groups (the groups instances of init_paths, the generators and the gather) on the same frame:
    `out` the oracle's bits, and the light's plane not empty."""
    import torch
    pipe, gp, p = _frame(pkg, boxes, 96, 64, 3)
    K = int(boxes["box"].desc.numLights)
    out = torch.full((64, 96, 4), SENTINEL, dtype=torch.float32, device=pipe.dev)
    g = torch.full((K + 1, 64, 96, 4), SENTINEL, dtype=torch.float32, device=pipe.dev)
    pipe.ctx.execute_light_groups(p, pipe.gb, C.c_void_p(out.data_ptr()), C.c_void_p(g.data_ptr()), pipe._stream_ptr())
    torch.cuda.synchronize()
    ref = _oracle(pkg, ob, boxes["box"], "box", pipe, gp, p, False)
    o, planes = out.cpu().numpy(), g.cpu().numpy()
    pipe.close()
    _same(o, ref, "light groups, out")
    assert not (planes == SENTINEL).any() and planes[0][..., :3].sum() > 0


@pytest.mark.gpu
def test_depth_12_context_runs_the_16_lane_generators(pkg, ob, boxes):
    """32 x 32 at depth 12: the generators run with G = 16 (two vertex records per 32 lanes more than at G = 8)."""
    _plain(pkg, ob, boxes, "box", 32, 32, 12)


@pytest.mark.gpu
def test_mis_power_reads_pos_n_pdf(pkg, ob, boxes):
    """BDPT_PARAM_MIS_POWER at 64 x 48, depth 4: mis_prefix_kernel reads pos, N and pdfForward through the accessors."""
    gpu, _ = _plain(pkg, ob, boxes, "box", 64, 48, 4, MIS_POWER)
    uniform, _ = _plain(pkg, ob, boxes, "box", 64, 48, 4, 0)
    assert not np.array_equal(gpu, uniform)  # the weights do something
