"""CPU checks of the masked-frame and adaptive-sampling interface: the ctypes structures and prototypes against
include/bdpt.h, and the Python binding's argument handling (adaptive_params, Context.adaptive_update, FramePipeline), so
that nothing a GPU would need is involved."""
import ctypes as C
import os
import re

import pytest

from binding_fakes import RecordingLib, context_without_device, header_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


STRUCTS = {
    "bdpt_adaptive_state": ["mean", "m2", "count", "mask", "active"],
    "bdpt_adaptive_params": ["threshold", "epsilon", "minSamples", "maxSamples", "blockSize"],
}


def test_adaptive_structs_match_the_header(pkg):
    a = pkg.abi
    lay = header_layout(STRUCTS, lang="c++")
    assert int(lay["bdpt_adaptive_state"]) == C.sizeof(a.AdaptiveState) == 40
    assert int(lay["bdpt_adaptive_params"]) == C.sizeof(a.AdaptiveParams) == 20
    for cls, cname in ((a.AdaptiveState, "bdpt_adaptive_state"), (a.AdaptiveParams, "bdpt_adaptive_params")):
        for name, _ in cls._fields_:
            assert int(lay[f"{cname}.{name}"]) == getattr(cls, name).offset, (cname, name)


def test_prototypes_match_the_header(pkg):
    """The three entry points are declared in the header with the argument counts abi.PROTOTYPES binds, and the built
    library exports them."""
    hdr = open(os.path.join(ROOT, "include", "bdpt.h")).read()
    for name, nargs in (("bdpt_execute_masked", 6), ("bdpt_adaptive_reset", 3), ("bdpt_adaptive_update", 5)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(pkg.abi.PROTOTYPES[name][1]), name
        assert hasattr(pkg.load_library(), name), name


def test_adaptive_params_defaults_and_overrides(pkg):
    d = pkg.ADAPTIVE_DEFAULTS
    a = pkg.adaptive_params()
    assert (a.minSamples, a.maxSamples, a.blockSize) == (d["min_samples"], d["max_samples"], d["block_size"])
    assert a.threshold == pytest.approx(d["threshold"]) and a.epsilon == pytest.approx(d["epsilon"])
    assert 2 <= a.minSamples <= a.maxSamples and a.blockSize in (1, 2, 4, 8, 16)
    b = pkg.adaptive_params({"threshold": -1.0, "min_samples": 2, "max_samples": 2, "block_size": 16})
    assert (b.threshold, b.minSamples, b.maxSamples, b.blockSize, b.epsilon) == (-1.0, 2, 2, 16, a.epsilon)


@pytest.mark.parametrize("bad, match", [
    ({"block_size": 3}, "block_size"),
    ({"block_size": 32}, "block_size"),
    ({"block_size": 0}, "block_size"),
    ({"min_samples": 1}, "min_samples"),
    ({"min_samples": 10, "max_samples": 9}, "min_samples"),
    ({"max_samples": 2 ** 32}, "32 bits"),
    ({"treshold": 0.1}, "unknown"),
])
def test_adaptive_params_refuses_bad_settings(pkg, bad, match):
    with pytest.raises(pkg.BdptError, match=match):
        pkg.adaptive_params(bad)


def _fake_context(pkg):
    """a Context whose library records what the adaptive entry points are handed"""
    return context_without_device(pkg, RecordingLib({
        "bdpt_adaptive_update": lambda p, state, frame, stream: ("update", p.threshold, p.epsilon, p.minSamples, p.maxSamples,
                                                                 p.blockSize, state.mean, frame),
        "bdpt_adaptive_reset": lambda state, stream: ("reset", state.mask),
        "bdpt_execute_masked": lambda params, gb, mask, out, stream: ("masked", mask, out),
    }, last_error=b"recorded"))


def test_context_passes_dict_params_and_pointers(pkg):
    ctx = _fake_context(pkg)
    st = pkg.abi.AdaptiveState(0x1000, 0x2000, 0x3000, 0x4000, 0x5000)
    ctx.adaptive_reset(st)
    ctx.adaptive_update({"threshold": 0.25, "block_size": 4}, st, C.c_void_p(0x6000))
    ctx.execute_masked(pkg.abi.Params(), pkg.abi.GBuffer(), C.c_void_p(0x4000), C.c_void_p(0x6000))
    reset, upd, masked = ctx._lib.calls
    assert reset == ("reset", 0x4000)
    assert upd[0] == "update" and upd[1] == pytest.approx(0.25) and upd[5] == 4 and upd[6] == 0x1000
    assert upd[3] == pkg.ADAPTIVE_DEFAULTS["min_samples"] and upd[4] == pkg.ADAPTIVE_DEFAULTS["max_samples"]
    assert masked[0] == "masked"
    with pytest.raises(pkg.BdptError, match="block_size"):
        ctx.adaptive_update({"block_size": 5}, st, C.c_void_p(0x6000))
    assert len(ctx._lib.calls) == 3  # (refused before the library saw it)


@pytest.mark.parametrize("kw", [dict(tile=(0, 32)), dict(stripes=(4, 2, 0)), dict(light_groups=True)])
def test_pipeline_refuses_adaptive_outside_whole_frames(pkg, kw):
    """Whole frames only, without light groups: refused before a GPU or the library is touched."""
    with pytest.raises(pkg.BdptError, match="adaptive sampling needs"):
        pkg.FramePipeline(None, 64, 64, adaptive={}, **kw)


def test_pipeline_refuses_bad_adaptive_settings_first(pkg):
    with pytest.raises(pkg.BdptError, match="min_samples"):
        pkg.FramePipeline(None, 64, 64, adaptive={"min_samples": 0})
