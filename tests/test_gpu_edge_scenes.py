"""bdpt_execute on the edge-case scenes of tests/edge_scenes.py against the CPU oracle (brute-force scan): the G-buffer
channels, the splat buffer words and the resolved image, bit for bit (every NaN counts as the same NaN), for two consecutive
frame counters, plain and with the stage-wise flags, one pipeline per case.  Then the invariances no other test holds on
degenerate content: occluder hints off, the number of lazy rounds, the masked frame, light groups, row bands.  And the
settled clampUpper rule (include/bdpt.h, bdpt_params): both sides refuse what the fixed-point splat conversion cannot hold."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import edge_scenes as es

pytestmark = pytest.mark.gpu

CASES = es.cases()
IDS = [c.id for c in CASES]
GB_NAMES = {"WorldPosition": "worldPosition", "WorldNormal": "worldNormal", "MaterialDiffuse": "materialDiffuse",
            "MaterialSpecRough": "materialSpecRough", "MaterialExtraParams": "materialExtra", "Emissive": "emissive"}
# the invariance tests: every family once at the largest frame, and every case of another depth
WIDE = [c for c in CASES if (c.W, c.H) == (33, 17) or c.depth != 3 or (c.family == "valid_counts" and c.variant.startswith("65"))]
WIDE_IDS = [c.id for c in WIDE]
SENTINEL = 7.0


def _words(a):
    """the words of a float32 array, every NaN as one NaN"""
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    a = np.ascontiguousarray(a, np.float32)
    w = a.view(np.uint32).copy()
    w[np.isnan(a)] = 0x7FC00000
    return w


def _same(a, b, label):
    x, y = _words(a).reshape(-1), _words(b).reshape(-1)
    assert x.shape == y.shape, label
    if not np.array_equal(x, y):
        bad = np.nonzero(x != y)[0]
        raise AssertionError(f"{label}: {len(bad)} words differ, first at {int(bad[0])}: {x[bad[0]]:#x} != {y[bad[0]]:#x}")


@contextlib.contextmanager
def _environ(**kw):
    """environment variables bdpt_resize reads (BDPT_NO_HINTS, BDPT_LAZY_ROUNDS), for the pipelines made inside"""
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _pipe(pkg, case, scene, **kw):
    pipe = pkg.FramePipeline(scene, case.W, case.H, max_depth=case.depth, mat_index=case.mat, clamp_upper=case.clamp,
                             min_t=case.min_t, flags=case.flags, **kw)
    if case.env:
        pipe.ctx.set_environment(color=es.ENV_COLOR)
    return pipe


def _upload_gbuffer(pipe, chan):
    """the caller-made G-buffer of a valid_counts case (oracle channel arrays) into the pipeline's tensors"""
    import torch
    for ch, on in GB_NAMES.items():
        t = torch.from_numpy(chan[on].reshape(pipe.H, pipe.W, 4)).to(pipe.dev)
        pipe.channels[ch].copy_(t.to(pipe.channels[ch].dtype))


def _render(pipe, case, frame, stage_flags, orc_chan=None):
    """one frame with the pipeline's counters set to frame number `frame` -> (image, splat words, counters)"""
    import torch
    pipe.gbuffer_frame, pipe.bdpt_frame = 0xdeadbeef + frame, 0x1337 + frame
    if case.valid is not None:
        _upload_gbuffer(pipe, orc_chan)
    pipe.render_frame(extra_flags=stage_flags, gbuffer=case.valid is None)
    torch.cuda.synchronize()
    return pipe.output.cpu().numpy().copy(), _splat_words(pipe), pipe.ctx.counters().as_dict()


def _splat_words(pipe):
    """the context's splat buffer, copied straight into host memory (a device-to-host hipMemcpy returns when the data is
    there; a device-to-device one into a tensor need not have landed when torch reads the tensor back)"""
    import torch
    ptr, n64 = pipe.ctx.splat_buffer()
    host = np.empty(n64, np.uint64)
    torch.cuda.synchronize()
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(ptr), C.c_size_t(n64 * 8), 2) == 0
    return host.reshape(-1, 4)


_oracle = {}


def _oracle_of(pkg, ob, case, frames=(0, 1)):
    key = (case.id, frames)
    if key not in _oracle:
        _oracle[key] = es.oracle_case(pkg, ob, case, frames=frames)
    return _oracle[key]


def test_pipeline_jitter_is_the_one_the_cameras_aim_with(pkg):
    assert pkg.msaa_jitter(0xdeadbeef) == es.JITTER0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_frame_equals_oracle_bit_for_bit(pkg, ob, case):
    """G-buffer, splat words and the resolved image of two frame counters, plain and stage by stage; the family's control"""
    ref = _oracle_of(pkg, ob, case)
    ok, seen = es.control_of(pkg, ob, case, ref)
    assert ok, ("the generator does not reach the family's branch", case.id, seen)
    scene = case.scene(pkg.abi)
    pipe = _pipe(pkg, case, scene)
    for frame in (0, 1):
        for stage, flags in es.STAGES:
            r = ref[frame, stage]
            img, spl, cnt = _render(pipe, case, frame, flags, r.chan)
            label = f"{case.id} frame {frame} {stage}"
            for ch, on in GB_NAMES.items():
                _same(pipe.channels[ch].float(), r.chan[on], f"{label}: {ch}")
            assert np.array_equal(spl, r.splat), f"{label}: splat words, {(spl != r.splat).any(axis=1).sum()} pixels differ"
            _same(img, r.image, f"{label}: image")
            for k in ("pixelsValid", "splatsLanded"):
                assert cnt[k] == r.cnt[k], (label, k, cnt[k], r.cnt[k])
            # every ray the oracle traces is traced, answered by a hint, or known to carry +0 (never more)
            assert cnt["raysLightExtend"] <= r.cnt["raysLightExtend"] and cnt["raysEyeExtend"] <= r.cnt["raysEyeExtend"], label
            assert cnt["raysNee"] + cnt["hintedNee"] <= r.cnt["raysNee"] and cnt["raysConnect"] <= r.cnt["raysConnect"], label
            if case.family == "camera" and case.variant == "away":
                assert all(cnt[k] == 0 for k in cnt if k.startswith("rays") and k != "raysPrimary"), cnt
            if case.family == "enclosed" and stage == "plain":
                assert cnt["raysConnectLazy"] > 0 and cnt["hintedNee"] > 0, cnt
                full = r.cnt["raysEyeExtend"] == r.cnt["pixelsValid"] * (case.depth - 1) and \
                    r.cnt["raysLightExtend"] == r.cnt["pixelsValid"] * case.depth
                if full:  # no vertex past a walk's end: every pair is a ray of its own, occluded, and so traced
                    assert cnt["raysConnect"] == r.cnt["raysConnect"], (cnt, r.cnt)
            if case.family == "origin" and case.depth == 16 and stage == "plain":
                assert cnt["raysConnectLazy"] > 0, cnt
            if stage == "connect" and not case.env:  # (with ENV_ON_MISS the eye walk's terms colour the pixel too)
                # what the oracle's connection image implies for the lazy rounds: a pixel is pending iff no non-zero pair was
                # visible (its RGB is +0); a pending pixel the oracle saturated found a visible zero-valued pair, which took at
                # least one lazy ray, and no pending pixel can take more than one ray per pair
                pend = (r.chan["worldPosition"][:, 3] != 0) & ~r.own[:, :3].view(np.uint32).any(axis=1)
                pairs = sum(min(t, case.depth - 1) for t in range(2, case.depth + 1))
                found = int((pend & (r.own[:, 3] == 1)).sum())
                assert found <= cnt["raysConnectLazy"] <= int(pend.sum()) * pairs, (label, found, cnt["raysConnectLazy"], int(pend.sum()), pairs)
    pipe.close()


def test_specular_flag_changes_the_frame(pkg, ob):
    """the control of `specular`: with BDPT_PARAM_SPECULAR_FROM_LOBE the specular bits chain and the image differs"""
    a, b = (next(c for c in CASES if c.family == "specular" and (c.W, c.H) == (33, 17) and c.flags == f) for f in (0, es.FROM_LOBE))
    ia, ib = _oracle_of(pkg, ob, a)[0, "plain"].image, _oracle_of(pkg, ob, b)[0, "plain"].image
    assert not np.array_equal(_words(ia), _words(ib))


@pytest.mark.parametrize("case", WIDE, ids=WIDE_IDS)
def test_hints_and_lazy_rounds_change_no_bit(pkg, ob, case):
    """BDPT_NO_HINTS, and BDPT_LAZY_ROUNDS 1, 2, 3 and 8 (both read by bdpt_resize): the same splat words and image as the
    oracle's; without hints no query is hinted, and the hinted queries are the rays the other run traced on top"""
    r = _oracle_of(pkg, ob, case)[0, "plain"]
    scene = case.scene(pkg.abi)
    seen = {}
    for label, env in (("default", {}), ("no hints", dict(BDPT_NO_HINTS=1)), ("rounds 1", dict(BDPT_LAZY_ROUNDS=1)),
                       ("rounds 2", dict(BDPT_LAZY_ROUNDS=2)), ("rounds 3", dict(BDPT_LAZY_ROUNDS=3)), ("rounds 8", dict(BDPT_LAZY_ROUNDS=8))):
        with _environ(**env):
            pipe = _pipe(pkg, case, scene)
        img, spl, cnt = _render(pipe, case, 0, 0, r.chan)
        pipe.close()
        assert np.array_equal(spl, r.splat), (case.id, label)
        _same(img, r.image, f"{case.id} {label}")
        seen[label] = cnt
    d, n = seen["default"], seen["no hints"]
    assert n["hintedNee"] == 0 and n["hintedSplat"] == 0
    assert d["raysNee"] + d["hintedNee"] == n["raysNee"] and d["raysSplat"] + d["hintedSplat"] == n["raysSplat"], (d, n)
    assert d["raysConnect"] == n["raysConnect"]
    if case.family == "enclosed":  # pending to exhaustion: every round count traces every candidate
        assert len({seen[k]["raysConnectLazy"] for k in seen}) == 1 and d["raysConnectLazy"] > 0, seen
    for k in ("rounds 1", "rounds 2", "rounds 3", "rounds 8"):  # (a round may trace more than the pixel needed, never fewer than one)
        assert (seen[k]["raysConnectLazy"] > 0) == (d["raysConnectLazy"] > 0), (k, seen[k], d)


@pytest.mark.parametrize("case", WIDE, ids=WIDE_IDS)
def test_masked_frame(pkg, ob, case):
    """bdpt_execute_masked: an all-ones mask is the plain frame; with an all-zeros mask only splats land (the splat words are
    the oracle's, `out` is untouched)"""
    import torch
    r = _oracle_of(pkg, ob, case)[0, "plain"]
    scene = case.scene(pkg.abi)
    pipe = _pipe(pkg, case, scene)
    img, spl, cref = _render(pipe, case, 0, 0, r.chan)
    p = pipe.last_params[1]
    for value in (1, 0):
        mask = torch.full((case.H, case.W), value, dtype=torch.uint8, device=pipe.dev)
        out = torch.full((case.H, case.W, 4), SENTINEL, dtype=torch.float32, device=pipe.dev)
        pipe.ctx.execute_masked(p, pipe.gb, C.c_void_p(mask.data_ptr()), C.c_void_p(out.data_ptr()), pipe._stream_ptr())
        torch.cuda.synchronize()
        cm = pipe.ctx.counters().as_dict()
        assert np.array_equal(_splat_words(pipe), r.splat), (case.id, value)
        if value:
            _same(out, r.image, f"{case.id}: all-ones mask")
            assert {k: cm[k] for k in cm if k.startswith("rays") or k.startswith("hinted")} == \
                   {k: cref[k] for k in cref if k.startswith("rays") or k.startswith("hinted")}
        else:
            assert (out.cpu().numpy() == SENTINEL).all(), case.id
            assert cm["splatsLanded"] == cref["splatsLanded"] and cm["raysNee"] == cm["raysConnect"] == cm["pixelsValid"] == 0
    pipe.close()


def _only(pkg, lights, k):
    out = []
    for i, l in enumerate(lights):
        m = pkg.abi.Light()
        C.memmove(C.byref(m), C.byref(l), C.sizeof(pkg.abi.Light))
        if i != k:
            m.intensity[0] = m.intensity[1] = m.intensity[2] = 0.0
        out.append(m)
    return out


GROUP_CASES = [c for c in WIDE if c.family in ("intensity", "black", "enclosed")]


@pytest.mark.parametrize("case", GROUP_CASES, ids=[c.id for c in GROUP_CASES])
def test_light_groups(pkg, ob, case):
    """bdpt_execute_light_groups, one group per light (the method of test_gpu_light_groups.py): `out` is the plain frame;
    plane k's RGB is the frame with only light k over the G-buffer without emission and background; the emission plane is the
    frame with every intensity zero; every plane's w is out's"""
    import torch
    r = _oracle_of(pkg, ob, case)[0, "plain"]
    scene = case.scene(pkg.abi)
    pipe = _pipe(pkg, case, scene)
    _render(pipe, case, 0, 0, r.chan)
    p, st = pipe.last_params[1], pipe._stream_ptr()
    K = int(scene.desc.numLights)
    lights = [scene.lights[i] for i in range(K)]
    new = lambda *s: torch.full(s + (case.H, case.W, 4), SENTINEL, dtype=torch.float32, device=pipe.dev)  # noqa: E731
    out, planes = new(), new(K + 1)
    pipe.ctx.execute_light_groups(p, pipe.gb, C.c_void_p(out.data_ptr()), C.c_void_p(planes.data_ptr()), st)
    torch.cuda.synchronize()
    _same(out, r.image, f"{case.id}: out")
    ch = pipe.channels
    dif0, em0 = ch["MaterialDiffuse"].clone(), ch["Emissive"].clone()
    em0[..., :3] = 0
    dif0[..., :3][ch["WorldPosition"][..., 3] == 0] = 0
    t = dict(ch)
    t["MaterialDiffuse"], t["Emissive"] = dif0, em0
    gb0 = pkg.abi.GBuffer(*[t[n].data_ptr() for n in GB_NAMES])
    for k in list(range(K)) + [None]:
        pipe.ctx.set_lights(_only(pkg, lights, k), st)
        ref = new()
        pipe.ctx.execute(p, gb0 if k is not None else pipe.gb, C.c_void_p(ref.data_ptr()), st)
        torch.cuda.synchronize()
        if k is None:
            _same(planes[K], ref, f"{case.id}: emission plane")
        else:
            _same(planes[k][..., :3], ref[..., :3], f"{case.id}: light plane {k}")
    pipe.ctx.set_lights(lights, st)
    for k in range(K + 1):
        _same(planes[k][..., 3], out[..., 3], f"{case.id}: plane {k} w")
    pipe.close()


BAND_CASES = [c for c in CASES if c.family in ("open", "light_at_camera") and (c.W, c.H) == (33, 17)]


@pytest.mark.parametrize("case", BAND_CASES, ids=[c.id for c in BAND_CASES])
def test_two_row_bands_equal_the_full_frame(pkg, ob, case):
    """two row bands with deferred resolve and summed splat buffers (the method of test_tiled_execution_equals_full_frame)"""
    import torch
    r = _oracle_of(pkg, ob, case)[0, "plain"]
    scene = case.scene(pkg.abi)
    bands = [(0, 7), (7, case.H)]
    pipes, splats = [_pipe(pkg, case, scene, tile=b) for b in bands], []
    for pp in pipes:
        buf = torch.zeros(case.W * case.H * 4, dtype=torch.int64, device="cuda")
        pp.ctx.set_splat_buffer(C.c_void_p(buf.data_ptr()), buf.numel())
        _, p = pp.render_frame(extra_flags=pkg.abi.PARAM_DEFER_RESOLVE | pkg.abi.PARAM_DEFER_TAIL)
        pp.ctx.execute_tail(p, pp.gb, C.c_void_p(pp.output.data_ptr()), pp._stream_ptr())
        torch.cuda.synchronize()
        splats.append(buf)
    total = splats[0] + splats[1]
    assert np.array_equal(total.cpu().numpy().view(np.uint64).reshape(-1, 4), r.splat), case.id
    img = np.zeros((case.H, case.W, 4), np.float32)
    for pp, (y0, y1) in zip(pipes, bands):
        pp.ctx.resolve(C.c_void_p(total.data_ptr()), 0, C.c_void_p(pp.output.data_ptr()))
        torch.cuda.synchronize()
        img[y0:y1] = pp.output.cpu().numpy()[y0:y1]
        pp.close()
    _same(img, r.image, case.id)


def test_clamp_upper_outside_the_fixed_point_range_is_refused(pkg, ob):
    """include/bdpt.h, bdpt_params: a NaN or negative clampUpper is BDPT_E_INVALID, one above BDPT_MAX_CLAMP_UPPER_SPLAT in a
    frame with splats BDPT_E_LIMIT, in bdpt_execute, _masked and _light_groups as in the oracle; without the splat stage +inf
    and FLT_MAX are taken, and the frame is the oracle's (the conversion of such a term is undefined on the host and different
    on the device: reverting the check makes the `intensity` frames at these bounds differ from the oracle's)"""
    import torch
    base = next(c for c in CASES if c.family == "intensity" and c.variant == "inf_nan_0" and (c.W, c.H) == (13, 5) and c.clamp == 1.0)
    scene = base.scene(pkg.abi)
    pipe = _pipe(pkg, base, scene)
    pipe.render_frame()
    torch.cuda.synchronize()
    st = pipe._stream_ptr()
    mask = torch.ones(base.H, base.W, dtype=torch.uint8, device=pipe.dev)
    planes = torch.zeros(4, base.H, base.W, 4, dtype=torch.float32, device=pipe.dev)
    out = C.c_void_p(pipe.output.data_ptr())
    above = float(np.nextafter(np.float32(es.CLAMP_LIMIT), np.float32(np.inf)))
    for clamp, code in ((float("nan"), -1), (-1.0, -1), (-float("inf"), -1), (above, -5), (es.FLT_MAX, -5), (float("inf"), -5)):
        pipe.clamp_upper = clamp
        p = pipe.bdpt_params()
        for call in (lambda: pipe.ctx.execute(p, pipe.gb, out, st),
                     lambda: pipe.ctx.execute_masked(p, pipe.gb, C.c_void_p(mask.data_ptr()), out, st),
                     lambda: pipe.ctx.execute_light_groups(p, pipe.gb, out, C.c_void_p(planes.data_ptr()), st)):
            with pytest.raises(pkg.BdptError, match=rf"\({code}\).*clampUpper"):
                call()
    pipe.close()
    for clamp in (es.FLT_MAX, float("inf"), es.CLAMP_LIMIT):
        case = es.Case("intensity", "inf_nan_0", 13, 5, 3, 1, flags=0 if clamp == es.CLAMP_LIMIT else es.NO_SPLAT, clamp=clamp)
        r = es.oracle_case(pkg, ob, case, stages=es.STAGES[:1])[0, "plain"]
        pipe = _pipe(pkg, case, scene)
        img, spl, _ = _render(pipe, case, 0, 0)
        assert np.array_equal(spl, r.splat), clamp
        _same(img, r.image, f"clampUpper {clamp}")
        pipe.close()
