"""GPU tests of bdpt_execute_masked and bdpt_adaptive_update / _reset (contract: include/bdpt.h "Masked frame" and
"Adaptive sampling").  Every comparison is bit for bit: masked frames against bdpt_execute on the same G-buffer and params
(and once against the CPU oracle), the update against a float32 numpy restatement of the header's arithmetic."""
import ctypes as C

import numpy as np
import pytest

from edge_images import _lum, np_update  # noqa: F401  (the float32 restatement lives with the other readings)

pytestmark = pytest.mark.gpu

RAY_KEYS = ("raysPrimary", "raysEyeExtend", "raysLightExtend", "raysNee", "raysSplat", "raysConnect", "pixelsValid",
            "splatsLanded", "raysConnectLazy", "hintedNee", "hintedSplat")
EXT = 1024 | 2048  # BDPT_PARAM_ENV_ON_MISS | BDPT_PARAM_EMISSIVE_HITS
MIS = 64           # BDPT_PARAM_MIS_POWER
SENTINEL = 7.0     # (a value no frame writes)
f32 = np.float32


def _bits(t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_bits(a, b, label):
    x, y = _bits(a), _bits(b)
    assert x.shape == y.shape, label
    if not np.array_equal(x, y):
        bad = (x != y).reshape(-1, x.shape[-1]).any(axis=-1).sum() if x.ndim > 1 else (x != y).sum()
        raise AssertionError(f"{label}: {bad} pixels differ")


@pytest.fixture(scope="module")
def atrium(pkg):
    scene = pkg.Scene.atrium(1, 262144)
    yield scene
    scene.close()


def _pipe(pkg, scene, W=256, H=144, D=8, mat=0, **kw):
    pipe = pkg.FramePipeline(scene, W, H, max_depth=D, mat_index=mat, **kw)
    pipe.ctx.set_environment(color=(0.3, 0.45, 0.7, 1.0))  # (what ENV_ON_MISS finds)
    return pipe


class Frame:
    """One pipeline's G-buffer of one frame; plain and masked renders of it with the same params."""

    def __init__(self, pkg, pipe, flags=0):
        import torch
        self.pkg, self.pipe, self.torch = pkg, pipe, torch
        self.gp = pipe.gbuffer_params()
        pipe.ctx.gbuffer_execute(self.gp, pipe.gb, pipe._stream_ptr())
        self.p = pipe.bdpt_params(flags)
        torch.cuda.synchronize()

    def _new(self):
        return self.torch.full((self.pipe.H, self.pipe.W, 4), SENTINEL, dtype=self.torch.float32, device=self.pipe.dev)

    def plain(self):
        out = self._new()
        self.pipe.ctx.execute(self.p, self.pipe.gb, C.c_void_p(out.data_ptr()), self.pipe._stream_ptr())
        self.torch.cuda.synchronize()
        return out, self.pipe.ctx.counters().as_dict()

    def masked(self, mask):
        m = self.torch.as_tensor(np.ascontiguousarray(mask, np.uint8), device=self.pipe.dev)
        out = self._new()
        self.pipe.ctx.execute_masked(self.p, self.pipe.gb, C.c_void_p(m.data_ptr()), C.c_void_p(out.data_ptr()),
                                     self.pipe._stream_ptr())
        self.torch.cuda.synchronize()
        return out, self.pipe.ctx.counters().as_dict()


def _check_masked(out, ref, mask, label):
    """Active pixels: bdpt_execute's bits; inactive ones: the sentinel."""
    o, r = out.cpu().numpy(), ref.cpu().numpy()
    act = np.asarray(mask) != 0
    _assert_bits(o[act], r[act], f"{label}: active pixels")
    assert (o[~act] == SENTINEL).all(), f"{label}: an inactive pixel was written"


def _block_mask(rng, H, W, frac, B=8):
    blocks = rng.random(((H + B - 1) // B, (W + B - 1) // B)) < frac
    return np.kron(blocks, np.ones((B, B), bool))[:H, :W].astype(np.uint8)


# ---- (1) all-ones mask = bdpt_execute ---------------------------------------------------------------------------------
VARIANTS = {
    "atrium ggx depth 8": dict(D=8, mat=0, flags=0),
    "lambert": dict(D=8, mat=1, flags=0),
    "mis power": dict(D=8, mat=0, flags=MIS),
    "env on miss + emissive hits": dict(D=8, mat=0, flags=EXT),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_all_ones_mask_equals_execute_atrium(pkg, atrium, name):
    v = VARIANTS[name]
    pipe = _pipe(pkg, atrium, D=v["D"], mat=v["mat"])
    f = Frame(pkg, pipe, v["flags"])
    ref, cref = f.plain()
    out, cm = f.masked(np.ones((pipe.H, pipe.W), np.uint8))
    _assert_bits(out, ref, name)
    assert {k: cm[k] for k in RAY_KEYS} == {k: cref[k] for k in RAY_KEYS}, name
    assert cref["raysNee"] > 0 and cref["raysConnect"] > 0 and cref["raysSplat"] > 0
    pipe.close()


@pytest.mark.parametrize("which", ["cornell depth 16", "courtyard alpha-masked"])
def test_all_ones_mask_equals_execute_other_scenes(pkg, which):
    scene = pkg.Scene.cornell() if which.startswith("cornell") else pkg.Scene.courtyard(3, 20000, 0.6)
    pipe = _pipe(pkg, scene, W=96, H=64, D=16 if which.startswith("cornell") else 6)
    f = Frame(pkg, pipe, 0)
    ref, cref = f.plain()
    out, cm = f.masked(np.ones((pipe.H, pipe.W), np.uint8))
    _assert_bits(out, ref, which)
    assert {k: cm[k] for k in RAY_KEYS} == {k: cref[k] for k in RAY_KEYS}, which
    pipe.close()
    scene.close()


# ---- (2) random masks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, MIS, MIS | EXT, EXT], ids=["plain", "mis", "mis+ext", "ext"])
@pytest.mark.parametrize("kind", ["blocks30", "pixels50"])
def test_random_masks(pkg, atrium, flags, kind):
    pipe = _pipe(pkg, atrium, W=200, H=120)
    rng = np.random.default_rng(11 if kind == "blocks30" else 12)
    mask = _block_mask(rng, pipe.H, pipe.W, 0.3) if kind == "blocks30" else (rng.random((pipe.H, pipe.W)) < 0.5).astype(np.uint8)
    f = Frame(pkg, pipe, flags)
    ref, cref = f.plain()
    out, cm = f.masked(mask)
    _check_masked(out, ref, mask, f"{kind} flags {flags}")
    for k in ("raysLightExtend", "raysSplat", "splatsLanded", "hintedSplat"):
        assert cm[k] == cref[k], k
    if flags & MIS:
        assert cm["raysEyeExtend"] == cref["raysEyeExtend"]
    else:
        assert 0 < cm["raysEyeExtend"] < cref["raysEyeExtend"]
    assert 0 < cm["raysNee"] < cref["raysNee"] and cm["pixelsValid"] < cref["pixelsValid"]
    pipe.close()


# ---- (3) all-zero mask ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, MIS])
def test_all_zero_mask(pkg, atrium, flags):
    pipe = _pipe(pkg, atrium, W=160, H=96)
    f = Frame(pkg, pipe, flags)
    ref, cref = f.plain()
    out, cm = f.masked(np.zeros((pipe.H, pipe.W), np.uint8))
    assert (out.cpu().numpy() == SENTINEL).all()
    for k in ("raysLightExtend", "raysSplat", "splatsLanded"):
        assert cm[k] == cref[k] > 0, k
    assert cm["raysNee"] == cm["raysConnect"] == cm["raysConnectLazy"] == cm["pixelsValid"] == 0
    if flags & MIS:
        assert cm["raysEyeExtend"] == cref["raysEyeExtend"] > 0
    else:
        assert cm["raysEyeExtend"] == 0
    pipe.close()


# ---- (4) against the CPU oracle ---------------------------------------------------------------------------------------
def test_masked_cornell_frame_against_oracle(pkg, ob):
    scene = pkg.Scene.cornell()
    pipe = _pipe(pkg, scene, W=64, H=64, D=4)
    f = Frame(pkg, pipe, 0)
    mask = _block_mask(np.random.default_rng(5), 64, 64, 0.5, 4)
    out, _ = f.masked(mask)
    orc = ob.OracleRender(pkg.abi, scene.desc, pipe.W, pipe.H)
    orc.gbuffer(pipe.cam, f.gp)
    orc.bdpt(pipe.cam, f.p)
    orc.resolve()
    ref = orc.image()
    orc.close()
    act = mask != 0
    _assert_bits(out.cpu().numpy()[act], ref[act], "oracle, active pixels")
    assert (out.cpu().numpy()[~act] == SENTINEL).all()
    pipe.close()
    scene.close()


# ---- (5) the update against numpy ------------------------------------------------------------------------------------
def _state(torch, mean, m2, count, mask):
    d = {"mean": torch.tensor(mean, device="cuda"), "m2": torch.tensor(m2, device="cuda"),
         "count": torch.tensor(count.view(np.int32), device="cuda"), "mask": torch.tensor(mask, device="cuda"),
         "active": torch.zeros(1, dtype=torch.int32, device="cuda")}
    return d


def _cstate(pkg, d):
    return pkg.abi.AdaptiveState(*[d[k].data_ptr() for k in ("mean", "m2", "count", "mask", "active")])


@pytest.fixture(scope="module")
def small_ctx(pkg):
    """A whole-frame context of 67 x 45 (not a multiple of any block) with a scene."""
    scene = pkg.Scene.cornell()
    ctx = pkg.Context(0)
    ctx.resize(67, 45, 0, 45, 3)
    ctx.set_scene(scene.desc)
    ctx.set_camera(scene.camera(67 / 45))
    yield ctx
    ctx.close()
    scene.close()


@pytest.mark.parametrize("B", [1, 2, 4, 8, 16])
def test_update_equals_numpy(pkg, small_ctx, B):
    import torch
    H, W = 45, 67
    rng = np.random.default_rng(100 + B)
    mn, mx, thr, eps = 4, 9, 0.2, 1e-3
    for it in range(3):
        mean = rng.random((H, W, 4), dtype=np.float32) * f32(0.8)
        frame = (mean + (rng.random((H, W, 4), dtype=np.float32) - f32(0.5)) * f32(0.3)).astype(f32)
        count = rng.integers(0, mx + 2, (H, W)).astype(np.uint32)   # 0 .. maxSamples + 1: both bounds are hit
        count[rng.random((H, W)) < 0.2] = mn - 1
        m2 = (rng.random((H, W), dtype=np.float32) * f32(0.05) * count.astype(f32)).astype(f32)
        m2[rng.random((H, W)) < 0.3] = 0.0  # (converges at minSamples)
        count[:, :40] = mx  # (a region of converged pixels: whole blocks of every size turn inactive)
        mask = (rng.random((H, W)) < 0.7).astype(np.uint8)
        exp = np_update(mean, m2, count, mask, frame, thr, eps, mn, mx, B)
        d = _state(torch, mean, m2, count, mask)
        fr = torch.tensor(frame, device="cuda")
        small_ctx.adaptive_update({"threshold": thr, "epsilon": eps, "min_samples": mn, "max_samples": mx, "block_size": B},
                                  _cstate(pkg, d), C.c_void_p(fr.data_ptr()))
        torch.cuda.synchronize()
        _assert_bits(d["mean"], exp[0], f"B {B}: mean")
        _assert_bits(d["m2"], exp[1], f"B {B}: m2")
        assert np.array_equal(d["count"].cpu().numpy().view(np.uint32), exp[2]), f"B {B}: count"
        assert np.array_equal(d["mask"].cpu().numpy(), exp[3]), f"B {B}: mask"
        assert int(d["active"].item()) == exp[4], f"B {B}: active"
        _assert_bits(fr, exp[5], f"B {B}: frame")
        assert 0 < exp[4] < H * W  # (the case is not trivial)


def test_reset(pkg, small_ctx):
    import torch
    H, W = 45, 67
    d = _state(torch, np.ones((H, W, 4), f32), np.ones((H, W), f32), np.full((H, W), 5, np.uint32), np.zeros((H, W), np.uint8))
    small_ctx.adaptive_reset(_cstate(pkg, d))
    torch.cuda.synchronize()
    assert (d["mean"] == 0).all() and (d["m2"] == 0).all() and (d["count"] == 0).all() and (d["mask"] == 1).all()
    assert int(d["active"].item()) == H * W


# ---- (6) a never-converging update is bdpt_accumulate --------------------------------------------------------------------
def test_never_converging_update_is_accumulate(pkg, small_ctx):
    import torch
    H, W = 45, 67
    rng = np.random.default_rng(7)
    d = _state(torch, np.zeros((H, W, 4), f32), np.zeros((H, W), f32), np.zeros((H, W), np.uint32), np.ones((H, W), np.uint8))
    small_ctx.adaptive_reset(_cstate(pkg, d))
    last = torch.zeros(H, W, 4, dtype=torch.float32, device="cuda")
    for k in range(12):
        frame = rng.random((H, W, 4), dtype=np.float32) * f32(3.0)
        a = torch.tensor(frame, device="cuda")
        b = torch.tensor(frame, device="cuda")
        small_ctx.adaptive_update({"threshold": -1.0, "min_samples": 2, "max_samples": 20, "block_size": 8}, _cstate(pkg, d),
                                  C.c_void_p(a.data_ptr()))
        small_ctx.accumulate(C.c_void_p(last.data_ptr()), C.c_void_p(b.data_ptr()), k, 100, H * W)
        torch.cuda.synchronize()
        _assert_bits(d["mean"], last, f"frame {k}: mean")
        _assert_bits(a, b, f"frame {k}: frame")
        assert int(d["active"].item()) == H * W
    assert (d["count"] == 12).all()


# ---- (7) end to end ---------------------------------------------------------------------------------------------------
def test_adaptive_loop_end_to_end(pkg):
    import torch
    scene = pkg.Scene.cornell()
    W, H, N = 64, 48, 24
    plain = _pipe(pkg, scene, W=W, H=H, D=3)
    frames = []
    for _ in range(N):
        plain.render_frame()
        torch.cuda.synchronize()
        frames.append(plain.output.cpu().numpy().copy())
    plain.close()
    settings = {"threshold": 0.05, "epsilon": 1e-3, "min_samples": 4, "max_samples": N, "block_size": 4}
    ad = _pipe(pkg, scene, W=W, H=H, D=3, adaptive=settings)
    assert ad.active_pixels() == W * H
    # the accumulate_kernel fold of the first k plain frames, for every k
    folds = [np.zeros((H, W, 4), f32)]
    for k, fr in enumerate(frames):
        folds.append(((f32(k) * folds[-1] + fr) / f32(k + 1)).astype(f32))
    active = [W * H]
    for i in range(N):
        ad.render_frame()
        active.append(ad.active_pixels())
        cnt = ad.adaptive_state["count"].cpu().numpy()
        mean = ad.adaptive_state["mean"].cpu().numpy()
        exp = np.take_along_axis(np.stack(folds), cnt[None, :, :, None].astype(np.int64), axis=0)[0]
        _assert_bits(mean, exp, f"frame {i}: mean = fold of the first count plain frames")
        _assert_bits(ad.output, mean, f"frame {i}: output shows the mean")
    assert all(b <= a for a, b in zip(active, active[1:])), active
    cnt = ad.adaptive_state["count"].cpu().numpy()
    assert cnt.min() < N and cnt.max() == N, "some pixels stop early, some run to maxSamples"
    assert active[-1] == 0
    ad.close()
    scene.close()


# ---- (8) graph capture ------------------------------------------------------------------------------------------------
def test_captured_masked_frame_and_update_replay(pkg, atrium):
    import torch
    K = 3
    settings = {"threshold": 0.3, "min_samples": 2, "max_samples": 8, "block_size": 8}
    H, W = 96, 160
    # a seeded state, so that the replayed frames (all of them the same frame: the graph's params are fixed) meet pixels
    # of every kind: converged, converging, capped
    rng = np.random.default_rng(3)
    seed = {"mean": torch.tensor(rng.random((H, W, 4), dtype=np.float32) * f32(0.5)),
            "m2": torch.tensor(rng.random((H, W), dtype=np.float32) * f32(0.2)),
            "count": torch.tensor(rng.integers(0, 8, (H, W)).astype(np.int32)),
            "mask": torch.tensor(_block_mask(rng, H, W, 0.6))}
    seed["count"][:, :64] = 8  # (capped: those blocks turn inactive)
    eager = _pipe(pkg, atrium, W=W, H=H, adaptive=settings)
    g0, b0 = eager.gbuffer_frame, eager.bdpt_frame
    for k, v in seed.items():
        eager.adaptive_state[k].copy_(v)
    for _ in range(K):
        eager.gbuffer_frame, eager.bdpt_frame = g0, b0
        eager.render_frame()
    torch.cuda.synchronize()
    ref = {k: v.clone() for k, v in eager.adaptive_state.items()}
    ref_out = eager.output.clone()
    assert 0 < int(ref["active"].item()) < W * H

    cap = _pipe(pkg, atrium, W=W, H=H, adaptive=settings)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cap.render_frame()  # (warm-up: launch grids sized outside the capture)
        cap.adaptive_reset()
    torch.cuda.synchronize()
    for k, v in seed.items():
        cap.adaptive_state[k].copy_(v)
    cap.gbuffer_frame, cap.bdpt_frame = g0, b0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        cap.render_frame()
        graph.capture_end()
    torch.cuda.synchronize()
    for _ in range(K):
        graph.replay()
    torch.cuda.synchronize()
    for k in ("mean", "m2"):
        _assert_bits(cap.adaptive_state[k], ref[k], f"replayed {k}")
    for k in ("count", "mask", "active"):
        assert torch.equal(cap.adaptive_state[k], ref[k]), f"replayed {k}"
    _assert_bits(cap.output, ref_out, "replayed output")
    del graph
    eager.close()
    cap.close()


# ---- (9) errors -------------------------------------------------------------------------------------------------------
def test_error_cases_on_a_real_context(pkg):
    import torch
    lib = pkg.load_library()
    scene = pkg.Scene.cornell()
    W, H = 64, 48
    out = torch.zeros(H, W, 4, dtype=torch.float32, device="cuda")
    mask = torch.ones(H, W, dtype=torch.uint8, device="cuda")
    d = _state(torch, np.zeros((H, W, 4), f32), np.zeros((H, W), f32), np.zeros((H, W), np.uint32), np.ones((H, W), np.uint8))
    st = _cstate(pkg, d)
    ctx = pkg.Context(0)
    p = pkg.abi.Params()
    p.maxDepth, p.clampUpper, p.minT = 3, 0.9, 1e-4
    gb = pkg.abi.GBuffer()
    good = pkg.adaptive_params({"min_samples": 2, "max_samples": 8, "block_size": 8})

    def masked(params=p, m=mask):
        return lib.bdpt_execute_masked(ctx._h, C.byref(params), C.byref(gb), None if m is None else C.c_void_p(m.data_ptr()),
                                       C.c_void_p(out.data_ptr()), None)

    def update(a=good, s=st):
        return lib.bdpt_adaptive_update(ctx._h, C.byref(a), None if s is None else C.byref(s), C.c_void_p(out.data_ptr()), None)

    assert masked() == -2 and update() == -2 and lib.bdpt_adaptive_reset(ctx._h, C.byref(st), None) == -2  # no scene, no size
    ctx.resize(W, H, 0, H, 3)
    assert masked() == -2 and update() == -2  # no scene
    ctx.set_scene(scene.desc)
    ctx.set_camera(scene.camera(W / H))
    assert masked(m=None) == -1
    assert update(s=None) == -1
    for field in ("mean", "m2", "count", "mask", "active"):
        s2 = _cstate(pkg, d)
        setattr(s2, field, None)
        assert update(s=s2) == -1, field
        assert lib.bdpt_adaptive_reset(ctx._h, C.byref(s2), None) == -1, field
    for fl in (pkg.abi.PARAM_DEFER_RESOLVE, pkg.abi.PARAM_DEFER_TAIL):
        q = pkg.abi.Params()
        C.pointer(q)[0] = p
        q.flags = fl
        assert masked(q) == -1
    for b in (0, 3, 5, 32):
        a = pkg.abi.AdaptiveParams(0.1, 1e-3, 2, 8, b)
        assert update(a) == -1, b
    assert update(pkg.abi.AdaptiveParams(0.1, 1e-3, 1, 8, 8)) == -1
    assert update(pkg.abi.AdaptiveParams(0.1, 1e-3, 9, 8, 8)) == -1
    assert update() == 0
    ctx.resize(W, H, 0, H // 2, 3)
    assert masked() == -1 and "whole frame" in lib.bdpt_last_error(ctx._h).decode()
    assert update() == -1
    ctx.resize_stripes(W, H, 4, 1, 0, 3)  # (stripes of one owner cover the frame, but they are still stripes)
    assert masked() == -1 and update() == -1
    torch.cuda.synchronize()
    ctx.close()
    scene.close()
