"""GPU tests of ambient occlusion (csrc/ao.hip): bdpt_ao_query and bdpt_ao_execute against the composed device loop they
replace (per sample sample_bsdf(mat_index=1) -> rays -> trace_rays("any") -> a count add, the LCG between the samples in
exact integer arithmetic) and against the CPU yardstick ao_reference.ao_oracle.  Every comparison is bit for bit: ao on its
float words viewed as integers, counts and states as integers, over every item."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ao_reference as ar
from area_scenes import LCG_INV, bits
from walk_loop import gpu, host

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
W, H = 64, 48
MISSES = 64  # miss records appended to the primary hits
MIN_T = 1e-4


def _lcg_torch(s):
    """one nextRand step on int32 states, in int64 so that nothing overflows"""
    import torch
    x = ((s.to(torch.int64) & 0xFFFFFFFF) * 1664525 + 1013904223) & 0xFFFFFFFF
    return torch.where(x >= 2**31, x - 2**32, x).to(torch.int32)


def ao_loop(ctx, surf, seeds, samples, radius, min_t=MIN_T, alive=None, stream=None):
    """The composed loop on the device, wholly on one stream: numpy in (surf (n, 24) float32, seeds (n,) uint32), numpy out
    (ao, counts, seeds_out) as bdpt_ao_query defines them.  The division is numpy's float32 one."""
    import torch
    surf_t, s = gpu(surf), gpu(np.ascontiguousarray(seeds, U).view(np.int32))
    n = surf_t.shape[0]
    live = surf_t.view(torch.int32)[:, 23] >= 0
    if alive is not None:
        live = live & (gpu(alive) != 0)
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    rays = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    rays[:, 0:3], rays[:, 3], rays[:, 7] = surf_t[:, 0:3], float(F(min_t)), float(F(radius))
    smp = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    vis = torch.empty(n, dtype=torch.uint8, device="cuda")
    for _ in range(samples):
        ctx.sample_bsdf(surf_t, s, mat_index=1, out=smp, stream=stream)
        rays[:, 4:7] = smp[:, 0:3]
        ctx.trace_rays(rays, "any", out=vis, stream=stream)
        cnt += ((vis != 0) & live).to(torch.int32)
        s = torch.where(live, _lcg_torch(_lcg_torch(s)), s)
    cnt = torch.where(live, cnt, torch.full_like(cnt, samples))
    torch.cuda.synchronize()
    counts = host(cnt).astype(U)
    return counts.astype(F) / F(samples), counts, host(s).view(U).copy()


def ao_query(ctx, surf, seeds, samples, radius, min_t=MIN_T, alive=None, count=None, fill=None):
    """one bdpt_ao_query with all three outputs -> numpy (ao, counts, seeds_out); fill: what the outputs hold before"""
    import torch
    n = len(surf)
    ao = torch.full((n,), -7.0 if fill is None else fill, dtype=torch.float32, device="cuda")
    counts = torch.full((n,), 77 if fill is None else int(fill), dtype=torch.int32, device="cuda")
    sout = torch.full((n,), 99 if fill is None else int(fill), dtype=torch.int32, device="cuda")
    res = ctx.ambient_occlusion(gpu(surf), gpu(np.ascontiguousarray(seeds, U).view(np.int32)), samples, radius, min_t=min_t,
                                alive=None if alive is None else gpu(alive), out=ao, counts=counts, seeds_out=sout, count=count)
    assert res is ao
    torch.cuda.synchronize()
    return host(ao), host(counts).view(U), host(sout).view(U)


def _assert_same(got, want, what):
    for name, g, w in zip(("ao", "counts", "seeds_out"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        diff = g.view(U) != w.view(U)
        assert not diff.any(), f"{what}: {name} differ in {int(diff.sum())} of {diff.size} items, first {int(np.argmax(diff))}"


def _primary_items(pipe):
    """bdpt_surface records of the pipeline's primary hits (camera_rays -> trace_rays -> shade_hits) with MISSES miss records
    appended, and one RNG state per item"""
    import torch
    rays = pipe.camera_rays()
    hits = torch.empty((W * H, 4), dtype=torch.float32, device="cuda")
    pipe.trace_rays(rays, "closest", out=hits)
    surf = pipe.shade_hits(rays, hits, normal_map=False)
    torch.cuda.synchronize()
    surf = host(surf)
    assert 0 < (surf.view(np.int32)[:, 23] >= 0).sum()
    rng = np.random.default_rng(17)
    miss = rng.uniform(-1, 1, (MISSES, 24)).astype(F)  # whatever a miss record holds: only its prim is looked at
    miss.view(np.int32)[:, 23] = -1 - np.arange(MISSES, dtype=np.int32) % 3
    surf = np.concatenate([surf, miss])
    seeds = rng.integers(0, 2**32, len(surf), dtype=np.uint64).astype(U)
    return surf, seeds


_state = {}


def _cornell(pkg, ob):
    if "cornell" not in _state:
        scene = pkg.Scene.cornell()
        pipe = pkg.FramePipeline(scene, W, H, max_depth=3, min_t=MIN_T)
        surf, seeds = _primary_items(pipe)
        lib = ob.load_oracle(pkg.abi)
        osc = lib.oracle_scene_create(C.byref(scene.desc))
        pos = np.ctypeslib.as_array(scene.desc.positions, (int(scene.desc.numVertices), 3))
        ext = float(np.max(pos.max(axis=0) - pos.min(axis=0)))
        _state["cornell"] = dict(scene=scene, pipe=pipe, surf=surf, seeds=seeds, lib=lib, osc=osc, ext=ext, loops={})
    return _state["cornell"]


def _loop_of(s, samples, radius):
    """the composed loop's answer, computed once per (S, radius) and shared"""
    key = (samples, repr(float(radius)))
    if key not in s["loops"]:
        s["loops"][key] = ao_loop(s["pipe"].ctx, s["surf"], s["seeds"], samples, radius)
    return s["loops"][key]


@pytest.mark.parametrize("samples", [1, 2, 7, 64])
def test_equals_the_loop_and_the_oracle(pkg, ob, samples):
    """(1) S x radius, and once minT >= radius: ao, counts and seedsOut of every item equal the composed device loop's and
    ao_oracle's"""
    s = _cornell(pkg, ob)
    ctx, surf, seeds = s["pipe"].ctx, s["surf"], s["seeds"]
    lv = surf.view(np.int32)[:, 23] >= 0
    assert (~lv).sum() >= MISSES
    for frac in (0.05, 0.25, float("inf")):
        radius = frac * s["ext"]
        got = ao_query(ctx, surf, seeds, samples, radius)
        _assert_same(got, _loop_of(s, samples, radius), f"S {samples} radius {frac}: the loop")
        orc = ar.ao_oracle(s["lib"], s["osc"], surf, seeds, samples, radius, MIN_T)
        _assert_same(got, (orc["ao"], orc["counts"], orc["seeds_out"]), f"S {samples} radius {frac}: the oracle")
        ao, counts, sout = got
        assert (ao[~lv] == 1.0).all() and (counts[~lv] == samples).all() and np.array_equal(sout[~lv], seeds[~lv])
        assert ((ao >= 0) & (ao <= 1)).all() and np.array_equal(sout[lv], ar.lcg_chain(seeds[lv], 2 * samples)[:, -1])
        if frac != 0.05 or samples > 2:
            assert (counts[lv] < samples).any()
        assert (counts[lv] > 0).any()
    # minT >= radius: every ray misses
    for radius, min_t in ((0.5, 0.5), (0.25, 1.0), (float("nan"), MIN_T)):
        ao, counts, sout = ao_query(ctx, surf, seeds, samples, radius, min_t=min_t)
        assert (ao == 1.0).all() and (counts == samples).all()
        assert np.array_equal(sout[lv], ar.lcg_chain(seeds[lv], 2 * samples)[:, -1])


def test_item_counts_device_counts_and_alive(pkg, ob):
    """(2) 1, 63, 64, 65 and 4099 items; device counts 0, 1, 63, 64, 65 and N with the outputs beyond the count untouched;
    alive bytes that drop every third item"""
    import torch
    s = _cornell(pkg, ob)
    ctx, radius, S = s["pipe"].ctx, 0.25 * s["ext"], 7
    n0 = len(s["surf"])
    pick = np.arange(4099) % n0
    surf, seeds = s["surf"][pick], (s["seeds"][pick] + (np.arange(4099) // n0).astype(U)).astype(U)
    want = ao_loop(ctx, surf, seeds, S, radius)
    for n in (1, 63, 64, 65, 4099):
        _assert_same(ao_query(ctx, surf[:n], seeds[:n], S, radius), [w[:n] for w in want], f"{n} items")
    n = len(surf)
    for m in (0, 1, 63, 64, 65, n, n + 9):
        cnt = torch.tensor([m], dtype=torch.int32, device="cuda")
        got = ao_query(ctx, surf, seeds, S, radius, count=cnt, fill=-7)
        k = min(m, n)
        _assert_same([g[:k] for g in got], [w[:k] for w in want], f"device count {m}")
        assert (got[0][k:] == -7.0).all() and (got[1].view(np.int32)[k:] == -7).all() and (got[2].view(np.int32)[k:] == -7).all(), m
    alive = (np.arange(n) % 3 != 1).astype(np.uint8)
    got = ao_query(ctx, surf, seeds, S, radius, alive=alive)
    _assert_same(got, ao_loop(ctx, surf, seeds, S, radius, alive=alive), "alive")
    dead = alive == 0
    assert (got[0][dead] == 1.0).all() and (got[1][dead] == S).all() and np.array_equal(got[2][dead], seeds[dead])
    orc = ar.ao_oracle(s["lib"], s["osc"], surf, seeds, S, radius, MIN_T, alive=alive)
    _assert_same(got, (orc["ao"], orc["counts"], orc["seeds_out"]), "alive: the oracle")
    # in place: seeds_out may be seeds
    st = gpu(seeds.view(np.int32))
    ctx.ambient_occlusion(gpu(surf), st, S, radius, min_t=MIN_T, seeds_out=st)
    torch.cuda.synchronize()
    assert np.array_equal(host(st).view(U), want[2])
    # host arrays go to the device and back
    h = ctx.ambient_occlusion(surf[:65], seeds[:65], S, radius, min_t=MIN_T)
    assert isinstance(h, np.ndarray) and np.array_equal(h.view(U), want[0][:65].view(U))


def test_alpha_masked_occluders(pkg, ob):
    """(3) a small courtyard with foliage cards: the any-hit alpha test runs inside the AO traversal"""
    import torch
    scene = pkg.Scene.courtyard(seed=1, target_triangles=4000, foliage_fraction=0.5)
    d = scene.desc
    alpha = [(d.materials[i].flags >> 17) & 3 for i in range(int(d.numMaterials))]
    assert 1 in alpha, "the scene has no alpha-masked material"
    pipe = pkg.FramePipeline(scene, W, H, max_depth=3, min_t=MIN_T)
    surf, seeds = _primary_items(pipe)
    pos = np.ctypeslib.as_array(d.positions, (int(d.numVertices), 3))
    ext = float(np.max(pos.max(axis=0) - pos.min(axis=0)))
    lib = ob.load_oracle(pkg.abi)
    osc = lib.oracle_scene_create(C.byref(d))
    for frac in (0.05, 0.25):
        got = ao_query(pipe.ctx, surf, seeds, 7, frac * ext)
        _assert_same(got, ao_loop(pipe.ctx, surf, seeds, 7, frac * ext), f"courtyard radius {frac}: the loop")
        orc = ar.ao_oracle(lib, osc, surf, seeds, 7, frac * ext, MIN_T)
        _assert_same(got, (orc["ao"], orc["counts"], orc["seeds_out"]), f"courtyard radius {frac}: the oracle")
        assert 0 < got[1].mean() < 7
    lib.oracle_scene_destroy(osc)
    torch.cuda.synchronize()
    pipe.close()
    scene.close()


def test_edge_records_beside_ordinary_ones(pkg, ob):
    """(4) N = 0, N not unit, NaN and +-inf in N or posW, subnormal posW, prim far out of range but >= 0, every fourth item
    of an ordinary batch: equal to the composed loop and the oracle, and every output in [0, 1]"""
    s = _cornell(pkg, ob)
    ctx, S = s["pipe"].ctx, 7
    surf, seeds = s["surf"].copy(), s["seeds"]
    nan, inf = F("nan"), F("inf")
    edges = [
        dict(N=(0, 0, 0)), dict(N=(-0.0, 0.0, -0.0)), dict(N=(0, 3.5, 0)), dict(N=(0.1, 0.2, 0.05)), dict(N=(1e-30, 1e-30, 1e-30)),
        dict(N=(1e20, 1e20, 0)), dict(N=(nan, 0, 1)), dict(N=(0, nan, 0)), dict(N=(inf, 0, 0)), dict(N=(0, -inf, 0)), dict(N=(inf, inf, inf)),
        dict(P=(nan, 100, 100)), dict(P=(100, 100, nan)), dict(P=(inf, 100, 100)), dict(P=(100, -inf, 100)),
        dict(P=(1e-40, 1e-41, 1e-45)), dict(P=(1e-40, 100, 1e-45)), dict(prim=2**31 - 1), dict(prim=123456789), dict(prim=0),
        dict(N=(nan, nan, nan), P=(nan, nan, nan)),
    ]
    where = np.nonzero(surf.view(np.int32)[:, 23] >= 0)[0][::4]
    for j, i in enumerate(where):
        e = edges[j % len(edges)]
        if "N" in e:
            surf[i, 4:7] = np.array(e["N"], F)
        if "P" in e:
            surf[i, 0:3] = np.array(e["P"], F)
        if "prim" in e:
            surf.view(np.int32)[i, 23] = e["prim"]
    assert len(where) >= 4 * len(edges)
    with np.errstate(all="ignore"):
        for frac in (0.25, float("inf")):
            radius = frac * s["ext"]
            got = ao_query(ctx, surf, seeds, S, radius)
            _assert_same(got, ao_loop(ctx, surf, seeds, S, radius), f"edge records, radius {frac}: the loop")
            # ... and to the oracle, but for the records whose normal is so short that a direction component is non-zero and
            # below 1e-30: the ray contract's one rule under which the tree walk and a linear scan may differ (the walk takes
            # such a component as zero; include/bdpt.h "Ray contract"), which the AO rays follow as every traced ray does
            orc = ar.ao_oracle(s["lib"], s["osc"], surf, seeds, S, radius, MIN_T)
            tiny = ((np.abs(orc["dirs"]) < 1e-30) & (orc["dirs"] != 0)).any(axis=(1, 2))
            assert tiny[where].sum() == sum(1 for j in range(len(where)) if edges[j % len(edges)].get("N") == (1e-30, 1e-30, 1e-30))
            assert not tiny[np.setdiff1d(np.arange(len(surf)), where)].any()
            _assert_same([g[~tiny] for g in got], [orc[k][~tiny] for k in ("ao", "counts", "seeds_out")],
                         f"edge records, radius {frac}: the oracle")
            ao, counts, sout = got
            assert np.isfinite(ao).all() and ((ao >= 0) & (ao <= 1)).all() and (counts <= S).all()
            # a zero or NaN normal, or a NaN position: every ray misses, after its 2 S draws
            for j, i in enumerate(where):
                e = edges[j % len(edges)]
                if e.get("N") in ((0, 0, 0), (-0.0, 0.0, -0.0)) or any(np.isnan(np.array(e.get("N", (0,)) + e.get("P", (0,)), F))):
                    assert ao[i] == 1.0 and counts[i] == S, (i, e)
                assert sout[i] == ar.lcg_chain(seeds[i:i + 1], 2 * S)[0, -1]
            # the ordinary items beside them are what they are without the edge records
            plain = _loop_of(s, S, radius)
            keep = np.ones(len(surf), bool)
            keep[where] = False
            _assert_same([g[keep] for g in got], [p[keep] for p in plain], "the items beside the edge records")


def _gbuffer_items(pipe, frame_count):
    """the query's inputs for the pass: positions, half-decoded normals, prim from worldPosition.w, and the pass's seeds"""
    pos = host(pipe.channels["WorldPosition"]).reshape(-1, 4)
    nrm = host(pipe.channels["WorldNormal"].float()).reshape(-1, 4)
    n = len(pos)
    rec = ar.surface_records(pos[:, 0:3], nrm[:, 0:3], np.where(pos[:, 3] != 0, 0, -1).astype(np.int32))
    st, _ = pipe.ctx.test_rng(np.arange(n, dtype=U), np.full(n, frame_count & 0xFFFFFFFF, U), 1)
    back = (st[:, 0].astype(np.uint64) + np.uint64(2**32 - 1013904223)) & np.uint64(0xFFFFFFFF)
    seeds = ((back * np.uint64(LCG_INV)) & np.uint64(0xFFFFFFFF)).astype(U)  # one LCG step back
    assert np.array_equal(ar.lcg(seeds), st[:, 0])
    return rec, seeds


def test_execute_equals_the_query_and_tiles_reproduce_the_frame(pkg, ob):
    """(5) bdpt_ao_execute equals the query fed the G-buffer; a rows tile and a stripes context write only their pixels, with
    the whole frame's values; the same frameCount twice gives the same bits, another differs"""
    import torch
    s = _cornell(pkg, ob)
    pipe, a = s["pipe"], pkg.abi
    st = pipe._stream_ptr()
    pipe.ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, st)
    torch.cuda.synchronize()
    radius, S = 0.25 * s["ext"], 7
    images = {}
    for frame in (0, 0, 5):
        pipe.ao_frame = frame
        img = host(pipe.ambient_occlusion(S, radius)).copy()
        assert pipe.ao_frame == frame + 1 and pipe.last_ao_params.frameCount == frame
        if frame in images:
            assert np.array_equal(bits(img), bits(images[frame]))
        images[frame] = img
    assert not np.array_equal(bits(images[0]), bits(images[5]))
    for frame, img in images.items():
        rec, seeds = _gbuffer_items(pipe, frame)
        ao, _, _ = ao_query(pipe.ctx, rec, seeds, S, radius)
        want = np.stack([ao, ao, ao, np.ones_like(ao)], axis=1).reshape(H, W, 4)
        assert np.array_equal(bits(img), bits(want)), frame
        orc = ar.ao_oracle(s["lib"], s["osc"], rec, seeds, S, radius, MIN_T)
        assert np.array_equal(bits(img[..., 0].reshape(-1)), bits(orc["ao"]))
        background = rec.view(np.int32)[:, 23] < 0
        assert background.any() and (ao[background] == 1.0).all() and (ao[~background] < 1.0).any()
    # tiles: other contexts on the same G-buffer
    p = a.AoParams(0, radius, MIN_T, S, 0)
    for kind in ("rows", "stripes"):
        ctx = pkg.Context(0)
        ctx.set_scene(s["scene"].desc)
        if kind == "rows":
            ctx.resize(W, H, 16, 32, 3)
        else:
            ctx.resize_stripes(W, H, 4, 3, 1, 3)
        rows = np.zeros(H, bool)
        for y0, y1 in ctx.row_ranges():
            rows[y0:y1] = True
        assert 0 < rows.sum() < H
        out = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
        ctx.ao_execute(p, pipe.gb, C.c_void_p(out.data_ptr()), st)  # (no camera set: the pass needs none)
        torch.cuda.synchronize()
        got = host(out)
        assert np.array_equal(bits(got[rows]), bits(images[0][rows])), kind
        assert (got[~rows] == -7.0).all(), kind
        ctx.close()


def test_after_a_geometry_update(pkg, ob):
    """(6) the short box moves (bdpt_update_geometry): AO equals the composed loop on the refitted tree, and differs from
    before"""
    import torch
    scene = pkg.Scene.cornell()
    pipe = pkg.FramePipeline(scene, W, H, max_depth=3, min_t=MIN_T)
    s = _cornell(pkg, ob)
    surf, seeds, radius, S = s["surf"], s["seeds"], 0.25 * s["ext"], 7
    before = ao_query(pipe.ctx, surf, seeds, S, radius)
    _assert_same(before, _loop_of(s, S, radius), "before the update")
    d = scene.desc
    pos = np.ctypeslib.as_array(d.positions, (int(d.numVertices), 3)).copy()
    pos[24:44] += np.array([-40.0, 0.0, -30.0], F)  # the five quads of the short block
    pipe.update_geometry(pos)
    after = ao_query(pipe.ctx, surf, seeds, S, radius)
    _assert_same(after, ao_loop(pipe.ctx, surf, seeds, S, radius), "after the update")
    assert not np.array_equal(after[1], before[1]) and np.array_equal(after[2], before[2])
    torch.cuda.synchronize()
    pipe.close()
    scene.close()


def _captured_once(enqueue, outputs, node_types):
    """test_gpu_walk_query.test_captured_emit_and_walk's sequence for `enqueue(stream)`: run it eagerly on a side stream,
    capture it into ONE kept graph (the only kept graph alive: it is deleted before this returns), check that capturing
    allocates nothing and runs nothing, read the graph's node types once, before any replay, and replay it twice.
    outputs: {name: tensor} the calls write."""
    import torch
    from test_gpu_walk_query import _graph_node_types
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        st = C.c_void_p(side.cuda_stream)
        enqueue(st)
        side.synchronize()
        eager = {k: t.clone() for k, t in outputs.items()}
        for t in outputs.values():
            t.fill_(-7)
        side.synchronize()
        pad = torch.zeros(1, device="cuda")
        trivial = torch.cuda.CUDAGraph()
        trivial.capture_begin()
        pad.add_(1)
        trivial.capture_end()
        alloc = torch.cuda.memory_allocated()
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        graph.capture_begin()
        enqueue(st)
        graph.capture_end()
        assert torch.cuda.memory_allocated() == alloc  # the calls allocate nothing
    torch.cuda.synchronize()
    for t in outputs.values():
        assert (t == -7).all()  # captured, not run
    assert _graph_node_types(graph) == node_types
    for _ in range(2):
        for t in outputs.values():
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        for k, t in outputs.items():
            assert torch.equal(t.view(torch.uint8), eager[k].view(torch.uint8)), k
    del graph, trivial
    return eager


def test_captured_gbuffer_and_ao_execute(pkg, ob):
    """(7) gbuffer_execute -> ao_execute captured into one graph: the G-buffer pass's kernel node and exactly one more for
    the AO call, nothing else; replays are identical to the eager run"""
    import torch
    s = _cornell(pkg, ob)
    pipe = s["pipe"]
    gp, p = pipe.gbuffer_params(), pkg.abi.AoParams(3, 0.25 * s["ext"], MIN_T, 7, 0)
    img = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")

    def enqueue(st):
        pipe.ctx.gbuffer_execute(gp, pipe.gb, st)
        pipe.ctx.ao_execute(p, pipe.gb, C.c_void_p(img.data_ptr()), st)

    eager = _captured_once(enqueue, dict(img=img), [0, 0])
    ao = host(eager["img"])
    assert (ao[..., 3] == 1.0).all() and (ao[..., 0] < 1.0).any() and (ao[..., 0] == 1.0).any()


def test_captured_ao_query(pkg, ob):
    """(7) ao_query alone, captured: exactly one kernel node; replays are identical to the eager run, which is the loop's"""
    import torch
    s = _cornell(pkg, ob)
    ctx, radius, S, n = s["pipe"].ctx, 0.25 * s["ext"], 7, len(s["surf"])
    surf, seeds = gpu(s["surf"]), gpu(s["seeds"].view(np.int32))
    outs = dict(ao=torch.zeros(n, dtype=torch.float32, device="cuda"), counts=torch.zeros(n, dtype=torch.int32, device="cuda"),
                sout=torch.zeros(n, dtype=torch.int32, device="cuda"))

    def enqueue(st):
        ctx.ambient_occlusion(surf, seeds, S, radius, min_t=MIN_T, out=outs["ao"], counts=outs["counts"], seeds_out=outs["sout"], stream=st)

    eager = _captured_once(enqueue, outs, [0])
    _assert_same([host(eager["ao"]), host(eager["counts"]).view(U), host(eager["sout"]).view(U)], _loop_of(s, S, radius), "eager")


def test_frames_and_counters_are_unchanged_by_ao(pkg):
    """(8) frame, AO calls on the pipeline's stream, frame gives the images of two frames without them, bit for bit; the
    counters and stage times the frame left are unchanged"""
    import torch
    scene = pkg.Scene.cornell()
    imgs, cnts = [], []
    for with_ao in (True, False):
        pipe = pkg.FramePipeline(scene, W, H, max_depth=4, flags=pkg.abi.PARAM_COUNTERS)
        pipe.ctx.enable_stage_timing(True)
        pipe.render_frame()
        torch.cuda.synchronize()
        first = host(pipe.output).copy()
        if with_ao:
            before, times = pipe.ctx.counters().as_dict(), pipe.ctx.stage_times()
            a1 = host(pipe.ambient_occlusion(8)).copy()
            surf, seeds = _primary_items(pipe)
            ao, _, _ = ao_query(pipe.ctx, surf, seeds, 4, 100.0)
            a2 = host(pipe.ambient_occlusion(64, radius=50.0))
            torch.cuda.synchronize()
            assert (a1[..., 0] < 1).any() and (ao < 1).any() and (a2[..., 0] < 1).any()
            assert pipe.ctx.counters().as_dict() == before
            assert pipe.ctx.stage_times() == times
        pipe.render_frame()
        torch.cuda.synchronize()
        imgs.append((first, host(pipe.output).copy()))
        cnts.append(pipe.ctx.counters().as_dict())
        pipe.close()
    for x, y in zip(imgs[0], imgs[1]):
        assert np.array_equal(bits(x), bits(y))
    assert cnts[0] == cnts[1]
    scene.close()


def test_error_cases_through_the_c_abi(pkg):
    """(9) every error case returns its code, bdpt_last_error names the call, and nothing is enqueued: the outputs keep their
    sentinel"""
    import torch
    a = pkg.abi
    lib = pkg.load_library()
    scene = pkg.Scene.cornell()
    ctx = pkg.Context(0)
    n = 256
    surf = torch.zeros((n, 24), dtype=torch.float32, device="cuda")
    seeds = torch.zeros(n, dtype=torch.int32, device="cuda")
    bytes_ = torch.ones(n, dtype=torch.uint8, device="cuda")
    cnt = torch.full((4,), n, dtype=torch.int32, device="cuda")
    outs = {k: torch.full((n,), -7, dtype=torch.int32, device="cuda") for k in ("ao", "c", "so")}
    img = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
    gpos = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    gnrm = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
    P = dict(sf=surf.data_ptr(), sd=seeds.data_ptr(), b=bytes_.data_ptr(), n=cnt.data_ptr(), img=img.data_ptr(), gp=gpos.data_ptr(),
             gn=gnrm.data_ptr(), **{k: t.data_ptr() for k, t in outs.items()})

    def q(h=ctx._h, num=n, samples=4, cnt=None, flags=0, reserved=0, sf=P["sf"], sd=P["sd"], al=None, ao=P["ao"], c=None, so=None, desc=True):
        d = a.AoDesc()
        d.num, d.samples, d.numDevice, d.radius, d.minT, d.flags, d.reserved = num, samples, cnt, 100.0, 1e-4, flags, reserved
        d.surfaces, d.seeds, d.alive, d.ao, d.counts, d.seedsOut = sf, sd, al, ao, c, so
        return lib.bdpt_ao_query(h, C.byref(d) if desc else None, None)

    def x(h=ctx._h, samples=4, reserved=0, gp=P["gp"], gn=P["gn"], out=P["img"], params=True, gbuffer=True):
        p = a.AoParams(0, 100.0, 1e-4, samples, reserved)
        gb = a.GBuffer()
        gb.worldPosition, gb.worldNormal = gp, gn
        return lib.bdpt_ao_execute(h, C.byref(p) if params else None, C.byref(gb) if gbuffer else None, out, None)

    assert q() == -2 and b"ao_query" in lib.bdpt_last_error(ctx._h)     # BDPT_E_STATE: no scene
    assert q(samples=0) == -2                                            # the state comes first
    assert x() == -2 and b"ao_execute" in lib.bdpt_last_error(ctx._h)
    ctx.set_scene(scene.desc)
    assert x() == -2 and b"ao_execute" in lib.bdpt_last_error(ctx._h)   # a scene but no size
    assert x(samples=0) == -2
    bad = [
        q(h=None), q(desc=False), q(samples=0), q(samples=65), q(samples=2**31), q(flags=1), q(flags=32), q(reserved=1),
        q(num=0, samples=0), q(num=0, flags=8), q(num=0, reserved=3),  # (found before the empty call returns)
        q(sf=None), q(sf=P["sf"] + 4), q(sd=None), q(sd=P["sd"] + 2), q(ao=None), q(ao=P["ao"] + 2), q(c=P["c"] + 1), q(so=P["so"] + 2),
        q(cnt=P["n"] + 2),
    ]
    assert all(rc == -1 for rc in bad), bad
    assert b"ao_query" in lib.bdpt_last_error(ctx._h)
    assert q(num=0, sf=None, sd=None, ao=None) == 0
    ctx.resize(W, H, 0, H, 3)
    bad = [x(h=None), x(params=False), x(gbuffer=False), x(samples=0), x(samples=65), x(reserved=1), x(gp=None), x(gp=P["gp"] + 8), x(gn=None),
           x(gn=P["gn"] + 4), x(out=None), x(out=P["img"] + 8)]
    assert all(rc == -1 for rc in bad), bad
    assert b"ao_execute" in lib.bdpt_last_error(ctx._h)
    torch.cuda.synchronize()
    for t in list(outs.values()) + [img]:
        assert (host(t) == -7).all()
    # and the good calls: every record at the origin with N = 0 misses; a zero worldPosition.w is the background
    assert q(al=P["b"], c=P["c"], so=P["so"], cnt=P["n"]) == 0 and q() == 0 and x() == 0  # (no camera: the pass needs none)
    torch.cuda.synchronize()
    assert (host(outs["ao"]).view(F) == 1.0).all() and (host(outs["c"]) == 4).all()
    assert (host(outs["so"]).view(U) == ar.lcg_chain(np.zeros(1, U), 8)[0, -1]).all()
    assert (host(img) == 1.0).all()
    ctx.close()
    scene.close()


def test_cpp_host_ao_equals_the_python_pipeline(pkg, tmp_path):
    """(10) bdpt_render --ao 4 --raw on the Cornell box, frame 0, equals FramePipeline.ambient_occlusion(4) with the host's
    defaults; --ao 0 and --ao 65 exit non-zero with a message"""
    import torch
    import __graft_entry__ as ge
    exe = os.path.join(ge.PKG_DIR, "host", "bdpt_render")
    assert os.path.exists(exe), "host/bdpt_render not built (run __graft_entry__.build())"
    raw = tmp_path / "ao.f32"
    r = subprocess.run([exe, "--scene", "cornell", "--width", str(W), "--height", str(H), "--frames", "1", "--ao", "4",
                        "--out", str(tmp_path / "ao.pfm"), "--raw", str(raw)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    cpp = np.fromfile(raw, F).reshape(H, W, 4)
    scene = pkg.Scene.cornell()
    pipe = pkg.FramePipeline(scene, W, H)
    pipe.ctx.gbuffer_execute(pipe.gbuffer_params(), pipe.gb, pipe._stream_ptr())
    img = pipe.ambient_occlusion(4)
    torch.cuda.synchronize()
    assert pipe.last_ao_params.frameCount == 0 and pipe.last_ao_params.radius == F(pkg.ao_default_radius(scene.desc))
    assert np.array_equal(bits(cpp), bits(host(img)))
    assert (cpp[..., 3] == 1.0).all() and (cpp[..., 0] < 1.0).any() and (cpp[..., 0] == 1.0).any()
    # an explicit radius reaches the pass
    r = subprocess.run([exe, "--scene", "cornell", "--width", str(W), "--height", str(H), "--frames", "1", "--ao", "4", "--ao-radius", "150",
                        "--out", str(tmp_path / "ao.pfm"), "--raw", str(raw)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    pipe.ao_frame = 0
    assert np.array_equal(bits(np.fromfile(raw, F).reshape(H, W, 4)), bits(host(pipe.ambient_occlusion(4, radius=150.0))))
    for n in ("0", "65"):
        r = subprocess.run([exe, "--ao", n], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--ao N" in r.stderr
    pipe.close()
    scene.close()
