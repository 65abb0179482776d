"""CPU checks of the walk query's interface (bdpt_walk_query): the ctypes structures and constants against include/bdpt.h,
and the Python binding's argument checks against a fake library, so that nothing a GPU would need is involved."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from binding_fakes import ROOT, FakeGpuTensor, RecordingLib, context_without_device, desc_fields, header_layout

STRUCTS = {
    "bdpt_walk_start": ("WalkStart", ["ray", "color", "unused"]),
    "bdpt_walk_info": ("WalkInfo", ["color", "status"]),
    "bdpt_walk_desc": ("WalkDesc", ["num", "steps", "numDevice", "matIndex", "flags", "minT", "reserved", "starts", "seeds", "first",
                                    "firstSpecular", "alive", "vertices", "info", "samples", "hits"]),
}
CONSTS = ["BDPT_WALK_SEED_PER_STEP", "BDPT_WALK_STATUS_STORED", "BDPT_WALK_STATUS_REAL", "BDPT_WALK_STATUS_SPECULAR",
          "BDPT_PARAM_SPECULAR_FROM_LOBE", "BDPT_MAX_DEPTH"]


def test_walk_structs_match_the_header(pkg):
    a = pkg.abi
    lay = header_layout(dict({c: f for c, (_, f) in STRUCTS.items()}, bdpt_light_emit=["ray", "color", "light"]),
                        {c: [c] for c in CONSTS})
    assert int(lay["bdpt_walk_start"]) == C.sizeof(a.WalkStart) == 48 == int(lay["bdpt_light_emit"])  # three float4
    assert int(lay["bdpt_walk_info"]) == C.sizeof(a.WalkInfo) == 16                                    # one float4
    for cname, (pyname, fields) in STRUCTS.items():
        cls = getattr(a, pyname)
        assert int(lay[cname]) == C.sizeof(cls), cname
        assert [n for n, _ in cls._fields_] == fields, cname
        for name in fields:
            assert int(lay[f"{cname}.{name}"]) == getattr(cls, name).offset, (cname, name)
    # emit_lights' output goes in as starts unchanged: the colour sits where bdpt_light_emit has it
    assert int(lay["bdpt_walk_start.color"]) == int(lay["bdpt_light_emit.color"]) == 32
    assert int(lay["bdpt_walk_start.unused"]) == int(lay["bdpt_light_emit.light"]) == 44
    assert (a.WalkInfo.color.offset, a.WalkInfo.status.offset) == (0, 12)  # the columns the binding documents
    got = [int(lay[c]) for c in CONSTS]
    assert got == [a.WALK_SEED_PER_STEP, a.WALK_STATUS_STORED, a.WALK_STATUS_REAL, a.WALK_STATUS_SPECULAR, a.PARAM_SPECULAR_FROM_LOBE,
                   a.BDPT_MAX_DEPTH] == [1, 1, 2, 4, 32, 16]


def test_the_entry_point_is_declared_exported_and_bound(pkg):
    a = pkg.abi
    src = open(os.path.join(ROOT, "include", "bdpt.h")).read()
    assert re.search(r"int\s+bdpt_walk_query\(bdpt_ctx\*\s*\w+,\s*const bdpt_walk_desc\*\s*\w+,\s*void\*\s*\w+\);", src)
    assert src.index("Connection queries:") < src.index("---- Walk queries") < src.index("int bdpt_walk_query(")
    assert a.PROTOTYPES["bdpt_walk_query"] == (C.c_int, [C.c_void_p, C.POINTER(a.WalkDesc), C.c_void_p])
    assert hasattr(C.CDLL(a.LIB_PATH), "bdpt_walk_query")
    lib = pkg.load_library()
    assert lib.bdpt_walk_query.argtypes == a.PROTOTYPES["bdpt_walk_query"][1] and lib.bdpt_walk_query.restype is C.c_int
    assert lib.bdpt_walk_query(None, None, None) == -1  # BDPT_E_INVALID: a NULL context needs no GPU


def _context_without_device(pkg, device=0):
    """a Context whose library records what the entry point is handed"""
    return context_without_device(pkg, RecordingLib({"bdpt_walk_query": lambda d, stream: desc_fields(d)}), device)


def test_good_calls_reach_the_library(pkg):
    import torch
    a = pkg.abi
    ctx = _context_without_device(pkg)
    f32, i32, u32, u8 = torch.float32, torch.int32, torch.uint32, torch.uint8
    n, steps = 70, 5
    starts, seeds = FakeGpuTensor((n, 12), f32, ptr=0x10000), FakeGpuTensor((n,), u32, ptr=0x20000)
    first, fspec, alive = FakeGpuTensor((n, 24), i32, ptr=0x30000), FakeGpuTensor((n,), u8, ptr=0x40000), FakeGpuTensor((n,), u8, ptr=0x50000)
    out = (FakeGpuTensor((steps, n, 24), f32, ptr=0x60000), FakeGpuTensor((steps, n, 4), i32, ptr=0x70000))
    smp, hits = FakeGpuTensor((steps, n, 8), f32, ptr=0x80000), FakeGpuTensor((steps, n, 4), f32, ptr=0x90000)
    cnt = FakeGpuTensor((1,), i32, ptr=0xa0000)
    res = ctx.walk(starts, seeds, steps, mat_index=1, min_t=0.25, from_lobe=True, first=first, first_specular=fspec, alive=alive, out=out,
                   samples=smp, hits=hits, count=cnt)
    assert res[0] is out[0] and res[1] is out[1]
    assert ctx._lib.calls[-1] == dict(
        num=n, steps=steps, numDevice=0xa0000, matIndex=1, flags=a.PARAM_SPECULAR_FROM_LOBE, minT=0.25, reserved=0, starts=0x10000,
        seeds=0x20000, first=0x30000, firstSpecular=0x40000, alive=0x50000, vertices=0x60000, info=0x70000, samples=0x80000, hits=0x90000)
    # one state per step: (steps, N) seeds and the flag
    per_step = FakeGpuTensor((steps, n), i32, ptr=0xb0000)
    ctx.walk(starts, per_step, steps, seed_per_step=True, out=out)
    c = ctx._lib.calls[-1]
    assert (c["flags"], c["seeds"], c["matIndex"], c["minT"]) == (a.WALK_SEED_PER_STEP, 0xb0000, 0, np.float32(1e-4))
    assert [c[k] for k in ("numDevice", "first", "firstSpecular", "alive", "samples", "hits")] == [None] * 6
    ctx.walk(starts, per_step, steps, seed_per_step=True, from_lobe=True, out=out)
    assert ctx._lib.calls[-1]["flags"] == a.WALK_SEED_PER_STEP | a.PARAM_SPECULAR_FROM_LOBE
    # each optional tensor on its own
    for key, kw in (("first", dict(first=first)), ("firstSpecular", dict(first_specular=fspec)), ("alive", dict(alive=alive)),
                    ("samples", dict(samples=smp)), ("hits", dict(hits=hits)), ("numDevice", dict(count=cnt))):
        ctx.walk(starts, seeds, steps, out=out, **kw)
        c = ctx._lib.calls[-1]
        others = [k for k in ("numDevice", "first", "firstSpecular", "alive", "samples", "hits") if k != key]
        assert c[key] is not None and [c[k] for k in others] == [None] * 5 and c["flags"] == 0, key
    # the limits of steps
    for s in (1, 16):
        ctx.walk(starts, seeds, s, out=(FakeGpuTensor((s, n, 24), f32), FakeGpuTensor((s, n, 4), f32)))
        assert ctx._lib.calls[-1]["steps"] == s


def test_frame_pipeline_walk_passes_its_settings(pkg):
    """FramePipeline.walk hands Context.walk the pipeline's BSDF, min_t, SPECULAR_FROM_LOBE flag and stream"""
    import torch
    a = pkg.abi
    seen = {}

    class Ctx:
        def walk(self, *args):
            seen["args"] = args
            return (FakeGpuTensor((2, 4, 24), torch.float32), FakeGpuTensor((2, 4, 4), torch.float32))

    pipe = pkg.FramePipeline.__new__(pkg.FramePipeline)
    pipe.ctx, pipe.mat_index, pipe.min_t, pipe.flags, pipe.dev = Ctx(), 1, 0.5, a.PARAM_SPECULAR_FROM_LOBE | a.PARAM_COUNTERS, None
    pipe._stream_ptr = lambda: "stream"

    class Torch:
        class cuda:
            @staticmethod
            def current_stream(dev):
                return None

            @staticmethod
            def is_current_stream_capturing():
                return True  # keep_for_stream then touches nothing

    pipe.torch = Torch
    import unittest.mock as mock
    with mock.patch("torch.cuda.is_current_stream_capturing", lambda: True):
        pipe.walk("starts", "seeds", 2, seed_per_step=True, first="first", first_specular="fs", alive="alive", out="out", samples="smp",
                  hits="hits", count="cnt")
    assert seen["args"] == ("starts", "seeds", 2, 1, 0.5, True, True, "first", "fs", "alive", "out", "smp", "hits", "cnt", "stream")


def test_bad_arguments_are_refused_before_the_library(pkg):
    import torch
    ctx = _context_without_device(pkg)
    f32, i32, u32, u8 = torch.float32, torch.int32, torch.uint32, torch.uint8
    n, steps = 64, 3
    starts, seeds = FakeGpuTensor((n, 12), f32), FakeGpuTensor((n,), u32)
    good = dict(starts=starts, seeds=seeds, steps=steps)
    bad = [
        dict(good, starts=np.zeros((n, 12), np.float32)),                                  # a host array
        dict(good, seeds=np.zeros(n, np.uint32)),
        dict(good, starts=torch.zeros(n, 12)),                                             # a CPU tensor
        dict(good, seeds=torch.zeros(n, dtype=i32)),
        dict(good, starts=None), dict(good, seeds=None),                                   # required
        dict(good, starts=FakeGpuTensor((n, 12), f32, index=1)),                           # another GPU
        dict(good, starts=FakeGpuTensor((n, 12), torch.float64)),                          # dtype
        dict(good, starts=FakeGpuTensor((n, 8), f32)),                                     # record width
        dict(good, starts=FakeGpuTensor((n * 12,), f32)),                                  # rank
        dict(good, starts=FakeGpuTensor((n, 12), f32, contiguous=False)),                  # strides
        dict(good, seeds=FakeGpuTensor((n,), f32)),                                        # seeds dtype
        dict(good, seeds=FakeGpuTensor((n - 1,), u32)),                                    # seeds length
        dict(good, seeds=FakeGpuTensor((steps, n), u32)),                                  # per-step states without the flag
        dict(good, seed_per_step=True),                                                    # the flag without per-step states
        dict(good, seed_per_step=True, seeds=FakeGpuTensor((steps + 1, n), u32)),
        dict(good, seed_per_step=True, seeds=FakeGpuTensor((n, steps), u32)),
        dict(good, seeds=FakeGpuTensor((n,), u32, contiguous=False)),
        dict(good, steps=0), dict(good, steps=17), dict(good, steps=-1), dict(good, steps=2.0), dict(good, steps=True),
        dict(good, steps=None),
        dict(good, mat_index=2), dict(good, mat_index=True),                               # material model
        dict(good, first=FakeGpuTensor((n, 20), f32)),                                     # predecessor width
        dict(good, first=FakeGpuTensor((n - 1, 24), f32)),                                 # predecessor length
        dict(good, first=torch.zeros(n, 24)),                                              # predecessor on the host
        dict(good, first=FakeGpuTensor((n, 24), f32, contiguous=False)),
        dict(good, first_specular=FakeGpuTensor((n,), i32)),                               # specular bytes dtype
        dict(good, first_specular=FakeGpuTensor((n, 1), u8)),                              # specular bytes rank
        dict(good, first_specular=np.zeros(n, np.uint8)),
        dict(good, alive=FakeGpuTensor((n,), torch.bool)),                                 # alive dtype
        dict(good, alive=FakeGpuTensor((n + 1,), u8)),                                     # alive length
        dict(good, alive=FakeGpuTensor((n,), u8, index=1)),
        dict(good, out=FakeGpuTensor((steps, n, 24), f32)),                                # out: the pair
        dict(good, out=(FakeGpuTensor((steps, n, 24), f32),)),
        dict(good, out=(FakeGpuTensor((steps, n, 24), f32), None)),
        dict(good, out=(FakeGpuTensor((n, steps, 24), f32), FakeGpuTensor((steps, n, 4), f32))),   # plane order
        dict(good, out=(FakeGpuTensor((steps, n, 24), f32), FakeGpuTensor((steps, n, 3), f32))),   # info width
        dict(good, out=(FakeGpuTensor((steps - 1, n, 24), f32), FakeGpuTensor((steps - 1, n, 4), f32))),
        dict(good, out=(FakeGpuTensor((steps, n, 24), torch.float16), FakeGpuTensor((steps, n, 4), f32))),
        dict(good, out=(FakeGpuTensor((steps, n, 24), f32), FakeGpuTensor((steps, n, 4), f32, contiguous=False))),
        dict(good, out=(torch.zeros(steps, n, 24), torch.zeros(steps, n, 4))),                     # on the host
        dict(good, samples=FakeGpuTensor((steps, n, 4), f32)),                             # samples width
        dict(good, samples=FakeGpuTensor((n, 8), f32)),                                    # samples rank
        dict(good, hits=FakeGpuTensor((steps, n, 8), f32)),                                # hits width
        dict(good, hits=FakeGpuTensor((steps, n, 4), torch.int64)),
        dict(good, hits=torch.zeros(steps, n, 4)),
        dict(good, count=FakeGpuTensor((2,), u32)),                                        # count size
        dict(good, count=FakeGpuTensor((1,), torch.int64)),                                # count dtype
        dict(good, count=torch.ones(1, dtype=i32)),                                        # count on the host
        dict(starts=FakeGpuTensor((2**28, 12), f32), seeds=FakeGpuTensor((2**28,), u32), steps=16),  # steps * N >= 2^32
    ]
    for kw in bad:
        with pytest.raises(pkg.BdptError):
            ctx.walk(**kw)
    assert ctx._lib.calls == []
