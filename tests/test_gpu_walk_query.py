"""GPU tests of the walk query (csrc/walk_query.hip): bdpt_walk_query against the composed loop it replaces (walk_loop.py:
trace_rays -> shade_hits -> sample_bsdf per bounce) and against bdpt_execute, whose connection-only and splat-only frames
the walks must reproduce when they take the loop's place in the composition of test_gpu_connect_queries.py.  Every
comparison is bit for bit, on the float words viewed as integers, over every item and every step."""
import ctypes as C

import numpy as np
import pytest

import edge_rays as er
import test_gpu_connect_queries as cq
from area_scenes import bits
from walk_loop import REAL, SPECULAR, STORED, ContextQueries, PipeQueries, gpu, host, kinds, prim_of, walk_loop

pytestmark = pytest.mark.gpu

F = np.float32
EXTRA = 64  # items appended that start outside the scene, and as many again without a path


def _bounds(desc):
    pos = np.ctypeslib.as_array(desc.positions, shape=(int(desc.numVertices), 3))
    return pos.min(axis=0).astype(F), pos.max(axis=0).astype(F)


def _walk_inputs(s, eye):
    """(starts (N, 12), seeds (N,), alive (N,)) of the pass's eye walk (from the G-buffer vertex and its first sample) or light
    walk (emit_lights' records as they are), as test_gpu_connect_queries._setup starts them"""
    import torch
    if ("in", eye) in s:
        return s[("in", eye)]
    pipe, n, valid = s["pipe"], s["n"], s["valid"]
    seed0 = gpu(cq._pixel_states(pipe.ctx, n, s["p"].frameCount).view(np.int32))
    if eye:
        surf = s["eye"][0][1]
        s1 = host(pipe.sample_bsdf(gpu(surf), seed0))
        starts = np.zeros((n, 12), F)
        starts[:, 0:3], starts[:, 3], starts[:, 4:7], starts[:, 7], starts[:, 8:11] = surf[:, 0:3], F(pipe.min_t), s1[:, 0:3], F(1e38), s1[:, 4:7]
        seeds = host(seed0)
    else:
        seed_l = torch.empty(n, dtype=torch.int32, device="cuda")
        starts = host(pipe.emit_lights(seed0, seeds_out=seed_l))
        seeds = host(seed_l)
    s[("in", eye)] = (starts, seeds, valid.astype(np.uint8))
    return s[("in", eye)]


def _with_extras(s, starts, seeds, alive):
    """the real items, then EXTRA items outside the scene's bounds pointing away from it (ghosts at step 0), then EXTRA
    copies of real items with alive = 0"""
    lo, hi = _bounds(s["pipe"].scene.desc)
    rng = np.random.default_rng(5)
    out = np.zeros((EXTRA, 12), F)
    away = rng.uniform(0.2, 1.0, (EXTRA, 3)).astype(F)
    out[:, 0:3] = hi + (hi - lo) * (F(0.5) + away)
    out[:, 3], out[:, 4:7], out[:, 7], out[:, 8:11] = F(1e-4), away, F(1e38), rng.uniform(0.1, 1.0, (EXTRA, 3)).astype(F)
    live = np.nonzero(alive)[0][:EXTRA]
    assert len(live) == EXTRA
    st = np.concatenate([starts, out, starts[live]])
    sd = np.concatenate([seeds, rng.integers(0, 2**31, EXTRA).astype(np.int32), seeds[live]])
    al = np.concatenate([alive, np.ones(EXTRA, np.uint8), np.zeros(EXTRA, np.uint8)])
    return st, sd, al


def _run(walker, starts, seeds, steps, **kw):
    """one call with all four outputs -> numpy (vertices, info, samples, hits)"""
    import torch
    n = starts.shape[0]
    smp = torch.full((steps, n, 8), -7.0, dtype=torch.float32, device="cuda")
    hits = torch.full((steps, n, 4), -7.0, dtype=torch.float32, device="cuda")
    kw = {k: (gpu(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    v, info = walker(gpu(starts), gpu(seeds), steps, samples=smp, hits=hits, **kw)
    torch.cuda.synchronize()
    return host(v), host(info), host(smp), host(hits)


def _assert_equal(got, want, what):
    for name, g, w in zip(("vertices", "info", "samples", "hits"), got, want):
        diff = (bits(g) != bits(w)).any(axis=-1)
        assert not diff.any(), (f"{what}: {name} differ in {int(diff.sum())} of {diff.size} records, first (step, item) "
                                f"{tuple(int(x) for x in np.argwhere(diff)[0])}")


def _assert_kinds(info, steps, what):
    """REAL at every step; a ghost at every step (the items outside at step 0, then every path that leaves the scene);
    a vertex that does not exist at every step (the items without a path)"""
    real, ghost, none = kinds(info)
    counts = [(int(real[s].sum()), int(ghost[s].sum()), int(none[s].sum())) for s in range(steps)]
    print(f"{what}: (real, ghost, none) per step {counts}")
    assert all(r > 0 and n >= EXTRA for r, _, n in counts), counts
    assert ghost[0].sum() >= EXTRA
    return counts


CONFIGS = [("cornell", 0, False, (2, 3, 8, 16)), ("cornell", 1, False, (2, 3, 8)), ("cornell", 0, True, (2, 3, 8)),
           ("atrium", 0, False, (2, 3, 8)), ("atrium", 1, False, (2, 3, 8))]


@pytest.mark.parametrize("eye", [True, False], ids=["eye", "light"])
@pytest.mark.parametrize("which,mat,lobe,all_steps", CONFIGS)
def test_equals_the_composed_loop(pkg, which, mat, lobe, all_steps, eye):
    """One call's vertices, info, samples and hits equal the loop's per-step results, for the pass's eye and light walks with
    items outside the scene and items without a path appended.  The loop runs once, at the largest step count: a walk of
    fewer steps is its first planes."""
    s = cq._setup(pkg, which, mat, 3, lobe)
    pipe = s["pipe"]
    starts, seeds, alive = _with_extras(s, *_walk_inputs(s, eye))
    want = walk_loop(PipeQueries(pipe), starts, seeds, max(all_steps), alive=alive)
    counts = _assert_kinds(want[1], max(all_steps), f"{which} mat {mat} lobe {lobe} {'eye' if eye else 'light'} (loop)")
    assert all(g > 0 for _, g, _ in counts), counts  # both scenes are open: paths leave them at every bounce
    if lobe:
        assert (want[1].view(np.uint32)[..., 3] & SPECULAR).any()
    for steps in all_steps:
        got = _run(pipe.walk, starts, seeds, steps, alive=alive)
        _assert_equal(got, [w[:steps] for w in want], f"{which} mat {mat} lobe {lobe} steps {steps}")


def test_first_and_first_specular(pkg):
    """With `first`: the origin is its position (the start record's origin is not read), a ghost at step 0 copies the whole
    record with prim = max(prim, 0) and keeps first_specular; without alive every item has a path."""
    s = cq._setup(pkg, "cornell", 0, 3)
    pipe, n = s["pipe"], s["n"]
    starts, seeds, _ = _walk_inputs(s, True)
    rng = np.random.default_rng(9)
    first = s["eye"][0][1].copy()  # the G-buffer vertices: prim 0 where valid, -1 and zeros where not
    first[:, 3:23] = np.where(s["valid"][:, None], first[:, 3:23], rng.uniform(-1, 1, (n, 20)).astype(F))
    prim_of(first)[::7] = -3
    prim_of(first)[1::7] = 12345
    fspec = (rng.integers(0, 3, n)).astype(np.uint8)
    moved = starts.copy()
    moved[:, 0:3] = 1e6  # not read with `first`
    moved[::5, 7] = 0.0  # tmax <= tmin: a ghost at step 0
    want = walk_loop(PipeQueries(pipe), moved, seeds, 3, first=first, first_specular=fspec)
    got = _run(pipe.walk, moved, seeds, 3, first=first, first_specular=fspec)
    _assert_equal(got, want, "first")
    real, ghost, none = kinds(got[1])
    assert ghost[0, ::5].all() and real[0].any() and none[1, ::5].all()
    g0 = got[0][0, ::5]
    assert np.array_equal(bits(g0[:, 0:23]), bits(first[::5, 0:23])) and np.array_equal(prim_of(g0), np.maximum(prim_of(first[::5]), 0))
    spec0 = (got[1].view(np.uint32)[0, ::5, 3] & SPECULAR) != 0
    assert np.array_equal(spec0, fspec[::5] != 0) and spec0.any() and not spec0.all()


def _as_walk(s, eye, steps):
    """the walks of FramePipeline.walk in the form test_gpu_connect_queries._walk returns them"""
    starts, seeds, alive = _walk_inputs(s, eye)
    v, info, _, _ = _run(s["pipe"].walk, starts, seeds, steps, alive=alive)
    k0 = 1 if eye else 0
    old = s["eye" if eye else "light"]
    vertex, color, spec = {k0: old[0][k0]}, {k: c for k, c in old[1].items() if k <= k0}, {k0: old[2][k0]}
    real, ghost = {k0: old[3][k0]}, {k0: old[4][k0]}
    r, g, _ = kinds(info)
    for st in range(steps):
        k = k0 + 1 + st
        vertex[k], color[k] = v[st], np.ascontiguousarray(info[st, :, 0:3])
        spec[k] = ((info[st].view(np.uint32)[:, 3] & SPECULAR) != 0).astype(np.uint8)
        real[k], ghost[k] = r[st], g[st]
    return vertex, color, spec, real, ghost


@pytest.mark.parametrize("which,mat", [("cornell", 0), ("atrium", 1)])
def test_equals_the_pass(pkg, which, mat):
    """Both walks from FramePipeline.walk in place of the loop, then the composition of connect_vertices (every pair, the
    gather rule in numpy) and of connect_camera / splat_add: the pass's NO_NEE | NO_SPLAT frame and the splat buffer of its
    NO_NEE | NO_CONNECT | DEFER_RESOLVE frame, at depth 3."""
    import torch
    D = 3
    base = cq._setup(pkg, which, mat, D)
    s = {k: v for k, v in base.items() if k != "pairs"}
    s["eye"], s["light"] = _as_walk(base, True, D - 1), _as_walk(base, False, D)
    pipe, n, p, valid = s["pipe"], s["n"], s["p"], s["valid"]
    # --- connections: every pair in the pass's slot order, all rays traced, the gather rule
    out = s["start"].copy()
    sat, any_vis = np.zeros(n, bool), np.zeros(n, bool)
    for t, c, l in cq._pairs(D):
        eye, light, eprev, lprev, es, ls, aL, aE = cq._pair_inputs(s, c, l)
        smp = pipe.connect_vertices(gpu(eye), gpu(light), eye_prev=gpu(eprev), light_prev=gpu(lprev), eye_specular=gpu(es),
                                    light_specular=gpu(ls))
        vis = pipe.trace_rays(smp[:, 0:8].contiguous(), "any")
        torch.cuda.synchronize()
        smp = host(smp)
        with np.errstate(all="ignore"):
            term = cq._clamp_vec(((aL * smp[:, 8:11]) * aE) / F(t), s["hi"])
        term[~valid] = 0
        vis = (host(vis) != 0) & valid
        add = vis & (term != 0).any(axis=1)
        out[add, 0:3] = cq._saturate(out[add, 0:3] + term[add])
        out[add, 3] = cq._saturate(out[add, 3] + F(1))
        sat |= add
        any_vis |= vis
    only = any_vis & ~sat
    out[only, 0:3] = cq._saturate(out[only, 0:3] + F(0))
    out[only, 3] = cq._saturate(out[only, 3] + F(1))
    diff = (bits(out) != bits(s["conn_ref"])).any(axis=1)
    assert not diff.any(), f"{int(diff.sum())} of {n} pixels differ, first {int(np.argmax(diff))}"
    assert sat.any() and only.any()
    # --- light tracing: every real light vertex to the camera, the visible ones splatted
    vertex, color, spec, real, _ = s["light"]
    own = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    for t in range(D):
        rec = vertex[t + 1].copy()
        rec[~real[t + 1]] = 0
        prim_of(rec)[~real[t + 1]] = -1
        cr = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
        ci = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        cc = torch.zeros(1, dtype=torch.int32, device="cuda")
        cv = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        cam = pipe.connect_camera(gpu(rec), pixel_jitter=(p.pixelJitter[0], p.pixelJitter[1]), light_specular=gpu(spec[t + 1]),
                                  compact=(cr, ci, cc))
        pipe.trace_rays(cr, "any", out=cv, count=cc)
        term = cq._torch_clamped(torch, (gpu(color[t]) * cam[:, 8:11]) * cam[:, 11:12], t + 2, float(s["hi"]))
        values = torch.cat([term, torch.zeros((n, 1), device="cuda")], dim=1).contiguous()
        pipe.splat_add(own, cam.view(torch.int32)[:, 12].contiguous(), values, visible=cv, items=ci, count=cc)
    torch.cuda.synchronize()
    got = host(own).view(np.uint64)
    diff = (got != s["splat_ref"]).any(axis=1)
    assert not diff.any(), f"{int(diff.sum())} of {n} splat pixels differ, first {int(np.argmax(diff))}"
    assert int(got[:, 3].sum()) == s["splat_cnt"]["splatsLanded"] > 0


def test_seeds_per_step(pkg):
    """distinct states per step against the loop fed the same states; and not what one state per item gives"""
    s = cq._setup(pkg, "cornell", 0, 3)
    pipe = s["pipe"]
    starts, seeds, alive = _with_extras(s, *_walk_inputs(s, False))
    steps, n = 4, starts.shape[0]
    per_step = np.random.default_rng(3).integers(-2**31, 2**31, (steps, n)).astype(np.int32)
    per_step[0] = seeds
    want = walk_loop(PipeQueries(pipe), starts, per_step, steps, seed_per_step=True, alive=alive)
    got = _run(pipe.walk, starts, per_step, steps, seed_per_step=True, alive=alive)
    _assert_equal(got, want, "seed per step")
    _assert_kinds(got[1], steps, "seed per step")
    # step 0 draws from the same states: vertices 0 and 1 are those of one state per item, the sample at vertex 1 and what
    # follows are not
    same = _run(pipe.walk, starts, seeds, steps, alive=alive)
    assert np.array_equal(bits(same[0][0:2]), bits(got[0][0:2])) and np.array_equal(bits(same[2][0]), bits(got[2][0]))
    assert not np.array_equal(bits(same[2][1]), bits(got[2][1])) and not np.array_equal(bits(same[0][2]), bits(got[0][2]))


@pytest.mark.parametrize("name", er.SCENES)
def test_edge_rays(pkg, gpu_ctx, name):
    """The start rays are the mixed batch of edge_rays.py (NaN, inf, zero and denormal directions, signed zeros, tmax <= tmin,
    rays onto shared vertices and edges, among ordinary ones), two steps, against the loop."""
    c = er.case(pkg, name)
    gpu_ctx.set_scene(c.sc.desc)
    r = c.batch.rays
    n = len(r)
    assert n <= er.MAX_RAYS
    rng = np.random.default_rng(11)
    starts = np.zeros((n, 12), F)
    starts[:, 0:3], starts[:, 3], starts[:, 4:7], starts[:, 7] = r[:, 0:3], r[:, 6], r[:, 3:6], r[:, 7]
    starts[:, 8:11] = rng.uniform(0.1, 1.0, (n, 3)).astype(F)
    seeds = rng.integers(-2**31, 2**31, n).astype(np.int32)
    min_t = 1e-4 * c.sc.ext
    for mat in (0, 1):
        want = walk_loop(ContextQueries(gpu_ctx, mat, min_t), starts, seeds, 2)
        got = _run(lambda *a, **kw: gpu_ctx.walk(*a, mat_index=mat, min_t=min_t, **kw), starts, seeds, 2)
        _assert_equal(got, want, f"{name} mat {mat}")
        # step 0 is the trace the scan answers: the same primitive, the same t, u, v
        hit0 = got[3][0]
        bad = er.differs_from_scan(c, 0, hit0.view(np.int32)[:, 3].copy(), hit0[:, 0:3])
        assert not bad.any(), c.batch.tally(bad)
        real, ghost, none = kinds(got[1])
        assert ghost[0, c.batch.of("invalid")].all() and real[0].any() and ghost[1].any() and none[1].any()
        assert real[1].any() or name == "grid"  # (one plane: a path that leaves it cannot come back)


def test_device_count(pkg):
    """count= of 0, 1, 63, 64, 65 and N (and beyond): items below it as without a count, every output at or beyond it untouched"""
    import torch
    s = cq._setup(pkg, "cornell", 0, 3)
    pipe = s["pipe"]
    starts, seeds, alive = _walk_inputs(s, False)
    n, steps = s["n"], 3
    full = _run(pipe.walk, starts, seeds, steps, alive=alive)
    st, sd, al = gpu(starts), gpu(seeds), gpu(alive)
    for m in (0, 1, 63, 64, 65, n, n + 9):
        cnt = torch.tensor([m], dtype=torch.int32, device="cuda")
        outs = [torch.full((steps, n, w), -7, dtype=torch.int32, device="cuda") for w in (24, 4, 8, 4)]
        pipe.walk(st, sd, steps, alive=al, out=(outs[0], outs[1]), samples=outs[2], hits=outs[3], count=cnt)
        torch.cuda.synchronize()
        k = min(m, n)
        for name, o, f in zip(("vertices", "info", "samples", "hits"), outs, full):
            g = host(o)
            assert np.array_equal(g[:, :k].view(np.uint32), bits(f[:, :k])), (m, name)
            assert (g[:, k:] == -7).all(), (m, name)


def _graph_node_types(graph):
    """the node types of a captured graph (hipGraphNodeType; 0 = kernel)"""
    hip = C.CDLL("libamdhip64.so")
    g = C.c_void_p(graph.raw_cuda_graph())
    num = C.c_size_t(0)
    assert hip.hipGraphGetNodes(g, None, C.byref(num)) == 0
    nodes = (C.c_void_p * num.value)()
    assert hip.hipGraphGetNodes(g, nodes, C.byref(num)) == 0
    types = []
    for nd in nodes:
        t = C.c_int(-1)
        assert hip.hipGraphNodeGetType(C.c_void_p(nd), C.byref(t)) == 0
        types.append(t.value)
    return types


def test_captured_emit_and_walk(pkg):
    """emit_lights -> walk captured into one graph on a side stream: two kernel nodes and nothing else, capturing allocates
    nothing, and two replays both equal the eager results."""
    import torch
    s = cq._setup(pkg, "cornell", 0, 3)
    pipe, n = s["pipe"], s["n"]
    ctx = pipe.ctx
    steps = 3
    seed0 = gpu(cq._pixel_states(ctx, n, s["p"].frameCount).view(np.int32))
    alive = gpu(s["valid"].astype(np.uint8))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()

    def buffers():
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")  # noqa: E731
        return dict(em=z(n, 12), sl=torch.zeros(n, dtype=torch.int32, device="cuda"), v=z(steps, n, 24), info=z(steps, n, 4),
                    smp=z(steps, n, 8), hits=z(steps, n, 4))

    def loop(b, st):
        ctx.emit_lights(seed0, min_t=pipe.min_t, out=b["em"], seeds_out=b["sl"], stream=st)
        ctx.walk(b["em"], b["sl"], steps, min_t=pipe.min_t, alive=alive, out=(b["v"], b["info"]), samples=b["smp"], hits=b["hits"],
                 stream=st)

    with torch.cuda.stream(side):
        st = C.c_void_p(side.cuda_stream)
        eager, cap = buffers(), buffers()
        loop(eager, st)
        side.synchronize()
        pad = torch.zeros(1, device="cuda")
        trivial = torch.cuda.CUDAGraph()
        trivial.capture_begin()
        pad.add_(1)
        trivial.capture_end()
        alloc = torch.cuda.memory_allocated()
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        graph.capture_begin()
        loop(cap, st)
        graph.capture_end()
        assert torch.cuda.memory_allocated() == alloc  # the loop allocates nothing
    torch.cuda.synchronize()
    assert not cap["v"].any() and not cap["em"].any()  # captured, not run
    assert _graph_node_types(graph) == [0, 0]  # emit_lights' kernel and the walk's: no memset, no copy, no host node
    real, ghost, none = kinds(host(eager["info"]))
    assert real.all(axis=0).any() and ghost.any() and none.any()
    # the eager results are the light walk of the module's other tests
    starts, seeds, al = _walk_inputs(s, False)
    want = _run(pipe.walk, starts, seeds, steps, alive=al)
    _assert_equal([host(eager[k]) for k in ("v", "info", "smp", "hits")], want, "eager")
    for _ in range(2):
        for k in ("v", "info", "smp", "hits"):
            cap[k].fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        for k in cap:
            assert torch.equal(cap[k].view(torch.uint8), eager[k].view(torch.uint8)), k
    del graph, trivial


def test_frames_are_unchanged_by_the_walks(pkg):
    """frame, walk queries on the pipeline's stream, frame gives the image of two frames without them, bit for bit; counters
    and stage times the frame left are unchanged."""
    import torch
    W, H = 96, 64
    scene = pkg.Scene.atrium(3, 20000)
    imgs, cnts = [], []
    for with_queries in (True, False):
        pipe = pkg.FramePipeline(scene, W, H, max_depth=4, flags=pkg.abi.PARAM_COUNTERS)
        pipe.ctx.enable_stage_timing(True)
        pipe.render_frame()
        torch.cuda.synchronize()
        first = host(pipe.output).copy()
        if with_queries:
            before = pipe.ctx.counters().as_dict()
            times = pipe.ctx.stage_times()
            n = W * H
            seeds = gpu((np.arange(n, dtype=np.uint32) * np.uint32(747796405)).view(np.int32))
            sl = torch.empty(n, dtype=torch.int32, device="cuda")
            em = pipe.emit_lights(seeds, seeds_out=sl)
            _, info = pipe.walk(em, sl, 4)
            rays = pipe.camera_rays()
            cam = torch.cat([rays, torch.ones((n, 4), device="cuda")], dim=1).contiguous()
            _, info2 = pipe.walk(cam, seeds, 5, seed_per_step=False)
            torch.cuda.synchronize()
            assert (host(info).view(np.uint32)[..., 3] & REAL).any() and (host(info2).view(np.uint32)[..., 3] & REAL).any()
            assert pipe.ctx.counters().as_dict() == before
            assert pipe.ctx.stage_times() == times
        pipe.render_frame()
        torch.cuda.synchronize()
        imgs.append((first, host(pipe.output).copy()))
        cnts.append(pipe.ctx.counters().as_dict())
        pipe.close()
    for a, b in zip(imgs[0], imgs[1]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert cnts[0] == cnts[1]
    scene.close()


def test_error_cases_through_the_c_abi(pkg):
    """every error case returns its code, bdpt_last_error names the call, and nothing is enqueued: the outputs keep their
    sentinel"""
    import torch
    a = pkg.abi
    lib = pkg.load_library()
    scene = pkg.Scene.cornell()
    ctx = pkg.Context(0)
    n, steps = 256, 2
    starts = torch.zeros((n, 12), dtype=torch.float32, device="cuda")
    seeds = torch.zeros(n, dtype=torch.int32, device="cuda")
    first = torch.zeros((n, 24), dtype=torch.float32, device="cuda")
    bytes_ = torch.ones(n, dtype=torch.uint8, device="cuda")
    cnt = torch.full((4,), n, dtype=torch.int32, device="cuda")
    outs = {k: torch.full((steps, n, w), -7, dtype=torch.int32, device="cuda") for k, w in (("v", 24), ("i", 4), ("s", 8), ("h", 4))}
    P = dict(st=starts.data_ptr(), sd=seeds.data_ptr(), f=first.data_ptr(), b=bytes_.data_ptr(), c=cnt.data_ptr(),
             **{k: t.data_ptr() for k, t in outs.items()})

    def q(h=ctx._h, num=n, steps=steps, cnt=None, mat=0, flags=0, reserved=0, st=P["st"], sd=P["sd"], f=None, fs=None, al=None, v=P["v"],
          i=P["i"], s=None, hh=None, desc=True):
        d = a.WalkDesc()
        d.num, d.steps, d.numDevice, d.matIndex, d.flags, d.minT, d.reserved = num, steps, cnt, mat, flags, 1e-4, reserved
        d.starts, d.seeds, d.first, d.firstSpecular, d.alive, d.vertices, d.info, d.samples, d.hits = st, sd, f, fs, al, v, i, s, hh
        return lib.bdpt_walk_query(h, C.byref(d) if desc else None, None)

    assert q() == -2 and b"walk_query" in lib.bdpt_last_error(ctx._h)  # BDPT_E_STATE: no scene
    assert q(steps=0) == -2                                             # the state comes first
    ctx.set_scene(scene.desc)
    bad = [
        q(h=None), q(desc=False), q(steps=0), q(steps=17), q(mat=2), q(flags=2), q(flags=64), q(flags=1 | 32 | 4), q(reserved=1),
        q(num=2**31, steps=2), q(num=2**28, steps=16),
        q(num=0, steps=0), q(num=0, mat=2), q(num=0, flags=8), q(num=0, reserved=3),  # (found before the empty call returns)
        q(st=None), q(st=P["st"] + 4), q(sd=None), q(sd=P["sd"] + 2), q(v=None), q(v=P["v"] + 8), q(i=None), q(i=P["i"] + 4),
        q(f=P["f"] + 4), q(s=P["s"] + 8), q(hh=P["h"] + 4), q(cnt=P["c"] + 2),
    ]
    assert all(rc == -1 for rc in bad), bad
    assert b"walk_query" in lib.bdpt_last_error(ctx._h)
    assert q(num=0, st=None, sd=None, v=None, i=None) == 0
    torch.cuda.synchronize()
    for t in outs.values():
        assert (host(t) == -7).all()
    # and the good calls: zero directions miss at step 0 (a ghost at the origin, then nothing); every flag, every optional buffer
    assert q(flags=1 | 32, mat=1, steps=1, f=P["f"], fs=P["b"], al=P["b"], s=P["s"], hh=P["h"], cnt=P["c"]) == 0
    torch.cuda.synchronize()
    info = host(outs["i"]).view(np.uint32)
    assert (info[0, :, 3] == (STORED | SPECULAR)).all() and (info[0, :, 0:3] == 0).all() and (host(outs["i"])[1] == -7).all()
    assert (host(outs["v"])[0] == 0).all() and (host(outs["s"])[0] == 0).all() and (host(outs["h"])[0, :, 3] == -1).all()
    assert q() == 0
    torch.cuda.synchronize()
    info = host(outs["i"]).view(np.uint32)
    assert (info[0, :, 3] == STORED).all() and (info[1] == 0).all() and (host(outs["v"])[1, :, 23] == -1).all()
    ctx.close()
    scene.close()
