"""CPU checks of reservoir reuse (bdpt_reuse_query, bdpt_reuse_execute, bdpt_ris_execute_reservoirs): the ctypes structures
against include/bdpt.h, the Python binding against a fake library, the generator's inverse, and the estimator itself: its
expectation, enumerated in float64 over every candidate sequence, equals the clamped direct lighting exactly, and the
definition (tests/reuse_reference.py reuse_compose over the CPU oracle) converges to that enumeration."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest

import direct_reference as dr
import reuse_reference as ur
import ris_reference as rr
from binding_fakes import ROOT, FakeGpuTensor, RecordingLib, context_without_device, desc_fields, header_layout

F, U = np.float32, np.uint32
MIN_T = 1e-4
STRUCTS = {
    "bdpt_reuse_reservoir": ("ReuseReservoir", ["light", "status", "state", "W", "M"]),
    "bdpt_reuse_desc": ("ReuseDesc", ["num", "flags", "numDevice", "matIndex", "neighbors", "inM", "poolM", "maxM", "poolNum", "normalMin",
                                      "planeMax", "clampUpper", "minT", "reserved", "surfaces", "alive", "seeds", "in", "poolSurfaces",
                                      "poolAlive", "pool", "neighborIndex", "color", "seedsOut", "traced", "out"]),
    "bdpt_reuse_params": ("ReuseParams", ["frameCount", "clampUpper", "minT", "matIndex", "flags", "neighbors", "radius", "inM", "poolM", "maxM",
                                          "normalMin", "planeMax", "poolCameraPos", "reserved", "in", "poolGbuffer", "pool", "neighborIndex",
                                          "outReservoirs"]),
}


def test_reuse_structs_match_the_header(pkg):
    a = pkg.abi
    consts = {"CONSTS": ["BDPT_REUSE_MAX_NEIGHBORS", "BDPT_REUSE_MAX_M", "BDPT_REUSE_SAME_PIXEL", "BDPT_REUSE_MAX_RADIUS"]}
    lay = header_layout({c: f for c, (_, f) in STRUCTS.items()}, consts)
    for cname, (pyname, fields) in STRUCTS.items():
        cls = getattr(a, pyname)
        assert int(lay[cname]) == C.sizeof(cls), cname
        assert [n for n, _ in cls._fields_] == fields, cname
        for name in fields:
            assert int(lay[f"{cname}.{name}"]) == getattr(cls, name).offset, (cname, name)
    assert [C.sizeof(getattr(a, n)) for n in ("ReuseReservoir", "ReuseDesc", "ReuseParams")] == [16, 160, 104]
    assert [int(v) for v in lay["CONSTS"].split()] == [a.REUSE_MAX_NEIGHBORS, a.REUSE_MAX_M, a.REUSE_SAME_PIXEL, a.REUSE_MAX_RADIUS] \
        == [ur.MAX_NEIGHBORS, ur.MAX_M, 1, 1024]


def test_the_entry_points_are_declared_exported_and_bound(pkg):
    a = pkg.abi
    src = open(os.path.join(ROOT, "include", "bdpt.h")).read()
    assert re.search(r"int\s+bdpt_reuse_query\(bdpt_ctx\*\s*\w+,\s*const bdpt_reuse_desc\*\s*\w+,\s*void\*\s*\w+\);", src)
    assert re.search(r"int\s+bdpt_reuse_execute\(bdpt_ctx\*\s*\w+,\s*const bdpt_reuse_params\*\s*\w+,\s*const bdpt_gbuffer\*\s*\w+,"
                     r"\s*float\*\s*\w+,\s*void\*\s*\w+\);", src)
    assert re.search(r"int\s+bdpt_ris_execute_reservoirs\(", src)
    section = src[src.index("---- Reservoir reuse"):src.index("int bdpt_reuse_query(")]
    for text in ("4276115653", "u_j * wsum <= w", "(wsum / (float)Z) / t_i(y_sel)", "always taken", "Z == 0", "1 / Z"):
        assert text in section, text
    assert a.PROTOTYPES["bdpt_reuse_query"] == (C.c_int, [C.c_void_p, C.POINTER(a.ReuseDesc), C.c_void_p])
    assert a.PROTOTYPES["bdpt_reuse_execute"] == (C.c_int, [C.c_void_p, C.POINTER(a.ReuseParams), C.POINTER(a.GBuffer), C.c_void_p, C.c_void_p])
    raw = C.CDLL(a.LIB_PATH)
    assert all(hasattr(raw, n) for n in ("bdpt_reuse_query", "bdpt_reuse_execute", "bdpt_ris_execute_reservoirs"))
    lib = pkg.load_library()
    assert lib.bdpt_reuse_query(None, None, None) == -1 and lib.bdpt_reuse_execute(None, None, None, None, None) == -1
    assert lib.bdpt_ris_execute_reservoirs(None, None, None, None, None, None) == -1
    mk = open(os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "csrc", "Makefile")).read()
    assert " reuse.o " in mk
    # one text for a sample's value: the three kernels call the helpers, none restates them
    csrc = os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "csrc")
    code = "\n".join(line.split("//")[0] for line in open(os.path.join(csrc, "reuse.hip")).read().splitlines())
    assert "lightGiven<" in code and "areaNee(" not in code and "directIfVisible<" not in code and "getLightData(" not in code
    light = open(os.path.join(csrc, "device_light.hpp")).read()
    assert "return lightGiven<GGX, AREA>(" in light.split("BD f3 lightCandidate(")[1]


def _ctx(pkg, device=0):
    return context_without_device(pkg, RecordingLib({
        "bdpt_reuse_query": lambda d, stream: (desc_fields(d), stream),
        "bdpt_reuse_execute": lambda p, gb, out, stream: (desc_fields(p), gb, out, stream),
        "bdpt_ris_execute_reservoirs": lambda p, gb, out, res, stream: (desc_fields(p), gb, out, res, stream)}), device)


def test_good_calls_reach_the_library(pkg):
    import torch
    ctx = _ctx(pkg)
    f32, i32, u32, u8 = torch.float32, torch.int32, torch.uint32, torch.uint8
    n, P = 70, 90
    surf, seeds, res = FakeGpuTensor((n, 24), f32, ptr=0x10000), FakeGpuTensor((n,), u32, ptr=0x20000), FakeGpuTensor((n, 4), i32, ptr=0x30000)
    nbr, alive = FakeGpuTensor((n, 3), i32, ptr=0x40000), FakeGpuTensor((n,), u8, ptr=0x50000)
    ps, pr, pa = FakeGpuTensor((P, 24), f32, ptr=0x60000), FakeGpuTensor((P, 4), u32, ptr=0x70000), FakeGpuTensor((P,), u8, ptr=0x80000)
    out, so, trc = FakeGpuTensor((n, 4), f32, ptr=0x90000), FakeGpuTensor((n,), i32, ptr=0xA0000), FakeGpuTensor((n,), u32, ptr=0xB0000)
    ro, cnt = FakeGpuTensor((n, 4), u32, ptr=0xC0000), FakeGpuTensor((1,), i32, ptr=0xD0000)
    got = ctx.reuse_lighting(surf, seeds, res, neighbor_index=nbr, pool_surfaces=ps, pool_reservoirs=pr, pool_alive=pa, in_m=8, pool_m=4,
                             max_m=160, normal_min=0.5, plane_max=0.25, mat_index=0, area_lights=True, clamp=2.5, min_t=0.125, alive=alive,
                             out=out, seeds_out=so, traced=trc, reservoirs_out=ro, count=cnt, stream="st")
    assert got is out
    c, st = ctx._lib.calls[-1]
    want = dict(num=n, flags=4096, numDevice=0xD0000, matIndex=0, neighbors=3, inM=8, poolM=4, maxM=160, poolNum=P, normalMin=0.5, planeMax=0.25,
                clampUpper=2.5, minT=0.125, surfaces=0x10000, alive=0x50000, seeds=0x20000, poolSurfaces=0x60000, poolAlive=0x80000,
                pool=0x70000, neighborIndex=0x40000, color=0x90000, seedsOut=0xA0000, traced=0xB0000, out=0xC0000)
    assert st == "st" and {k: c[k] for k in want} == want and c["in"] == 0x30000 and list(c["reserved"]) == [0, 0]
    # the pool defaults to the items; without neighbours no pool is passed
    ctx.reuse_lighting(surf, seeds, res, neighbor_index=nbr, alive=alive, out=out)
    c, _ = ctx._lib.calls[-1]
    assert (c["poolSurfaces"], c["pool"], c["poolAlive"], c["poolNum"], c["maxM"]) == (0x10000, 0x30000, 0x50000, n, 1 << 24)
    assert c["normalMin"] == -math.inf and c["planeMax"] == math.inf and (c["inM"], c["poolM"], c["matIndex"], c["flags"]) == (0, 0, 1, 0)
    ctx.reuse_lighting(surf, seeds, res, out=out)
    c, _ = ctx._lib.calls[-1]
    assert (c["neighbors"], c["poolSurfaces"], c["pool"], c["neighborIndex"], c["poolNum"], c["out"]) == (0, None, None, None, 0, None)
    # the G-buffer calls
    ctx._frame = (2, 3)
    img, gb, gb2 = FakeGpuTensor((2, 3, 4), f32, ptr=0x1000), pkg.abi.GBuffer(), pkg.abi.GBuffer()
    rin, rpool, rout = FakeGpuTensor((2, 3, 4), i32, ptr=0x2000), FakeGpuTensor((2, 3, 4), i32, ptr=0x3000), FakeGpuTensor((2, 3, 4), i32, ptr=0x4000)
    p = ctx.reuse_execute(gb, img, rin, neighbors=1, same_pixel=True, pool_gbuffer=gb2, pool_reservoirs=rpool, pool_camera_pos=(1, 2, 3),
                          in_m=8, max_m=160, mat_index=0, clamp=1.5, min_t=0.5, frame_count=7, reservoirs_out=rout, stream="s")
    f, gb_seen, out_seen, st = ctx._lib.calls[-1]
    assert isinstance(p, pkg.abi.ReuseParams) and gb_seen is gb and (out_seen.value, st) == (0x1000, "s")
    assert (f["frameCount"], f["flags"], f["neighbors"], f["radius"], f["inM"], f["poolM"], f["maxM"], f["matIndex"]) == (7, 1, 1, 0, 8, 0, 160, 0)
    assert list(f["poolCameraPos"]) == [1.0, 2.0, 3.0] and (f["in"], f["pool"], f["neighborIndex"], f["outReservoirs"]) == (0x2000, 0x3000, None, 0x4000)
    assert C.addressof(p.poolGbuffer.contents) == C.addressof(gb2)
    p = ctx.reuse_execute(gb, img, rin, neighbors=4, radius=9, reservoirs_out=rout)
    assert (p.flags, p.neighbors, p.radius, p.pool, C.addressof(p.poolGbuffer.contents)) == (0, 4, 9, 0x2000, C.addressof(gb))
    rsv = FakeGpuTensor((2, 3, 2, 4), i32, ptr=0x5000)
    ctx.ris_execute(gb, img, candidates=4, samples=2, reservoirs=rsv, stream="s")
    f, _, out_seen, res_seen, st = ctx._lib.calls[-1]
    assert (f["candidates"], f["samples"], out_seen.value, res_seen.value, st) == (4, 2, 0x1000, 0x5000, "s")


def test_bad_arguments_are_refused_before_the_library(pkg):
    import torch
    ctx = _ctx(pkg)
    f32, i32, u32, u8 = torch.float32, torch.int32, torch.uint32, torch.uint8
    n = 64
    res = FakeGpuTensor((n, 4), i32, ptr=0x3000)
    good = dict(surfaces=FakeGpuTensor((n, 24), f32), seeds=FakeGpuTensor((n,), u32), reservoirs=res,
                neighbor_index=FakeGpuTensor((n, 2), i32))
    bad = [
        dict(good, reservoirs=FakeGpuTensor((n, 3), i32)), dict(good, reservoirs=FakeGpuTensor((n, 4), f32)),
        dict(good, neighbor_index=FakeGpuTensor((n, 9), i32)), dict(good, neighbor_index=FakeGpuTensor((n + 1, 2), i32)),
        dict(good, neighbor_index=FakeGpuTensor((n,), i32)), dict(good, neighbor_index=np.zeros((n, 2), U)),
        dict(good, pool_reservoirs=res), dict(good, pool_alive=FakeGpuTensor((n,), u8)),  # without pool_surfaces
        dict(good, pool_surfaces=FakeGpuTensor((9, 24), f32)), dict(good, pool_surfaces=FakeGpuTensor((9, 24), f32), pool_reservoirs=FakeGpuTensor((8, 4), i32)),
        dict(good, pool_surfaces=FakeGpuTensor((9, 24), f32), pool_reservoirs=FakeGpuTensor((9, 4), i32), pool_alive=FakeGpuTensor((9,), i32)),
        dict(good, neighbor_index=None, pool_surfaces=FakeGpuTensor((9, 24), f32), pool_reservoirs=FakeGpuTensor((9, 4), i32)),
        dict(good, in_m=-1), dict(good, pool_m=2**32), dict(good, max_m=2.0), dict(good, in_m=True), dict(good, normal_min=None),
        dict(good, plane_max="1"), dict(good, mat_index=2), dict(good, area_lights=1), dict(good, clamp=-1.0), dict(good, clamp=float("nan")),
        dict(good, reservoirs_out=res), dict(good, reservoirs_out=FakeGpuTensor((n, 3), i32)), dict(good, traced=FakeGpuTensor((n, 1), u32)),
        dict(good, pool_surfaces=FakeGpuTensor((9, 24), f32), pool_reservoirs=FakeGpuTensor((9, 4), i32, ptr=0x7000),
             reservoirs_out=FakeGpuTensor((n, 4), i32, ptr=0x7000)),
        dict(surfaces=np.zeros((n, 24), F), seeds=np.zeros(n, U), reservoirs=np.zeros((n, 4), U), neighbor_index=FakeGpuTensor((n, 2), i32)),
    ]
    for kw in bad:
        with pytest.raises(pkg.BdptError):
            ctx.reuse_lighting(**kw)
    gb, img, rin = pkg.abi.GBuffer(), FakeGpuTensor((2, 3, 4), f32), FakeGpuTensor((2, 3, 4), i32, ptr=0x2000)
    with pytest.raises(pkg.BdptError):
        ctx.reuse_execute(gb, img, rin)  # no frame size yet
    ctx._frame = (2, 3)
    for kw in (dict(neighbors=9), dict(neighbors=2), dict(neighbors=2, radius=1025), dict(neighbors=2, same_pixel=True),
               dict(neighbors=1, same_pixel=True, neighbor_index=FakeGpuTensor((2, 3, 1), i32)), dict(neighbors=1, same_pixel=1),
               dict(neighbors=2, neighbor_index=FakeGpuTensor((2, 3, 3), i32)), dict(mat_index=3), dict(clamp=-0.5), dict(pool_gbuffer="gb"),
               dict(pool_reservoirs=FakeGpuTensor((2, 3, 3), i32)), dict(reservoirs_out=rin), dict(max_m=-1)):
        with pytest.raises(pkg.BdptError):
            ctx.reuse_execute(gb, img, rin, **kw)
    for g, o, r in ((None, img, rin), (gb, FakeGpuTensor((2, 3, 3), f32), rin), (gb, img, FakeGpuTensor((2, 3, 4), f32))):
        with pytest.raises(pkg.BdptError):
            ctx.reuse_execute(g, o, r)
    with pytest.raises(pkg.BdptError):
        ctx.ris_execute(gb, img, candidates=4, samples=2, reservoirs=FakeGpuTensor((2, 3, 1, 4), i32))
    assert ctx._lib.calls == []


def test_prev_state_inverts_the_generator():
    """prev(next(s)) == s and next(prev(s)) == s on the pinned states of test_ris_cpu.py and 4096 random ones"""
    pinned = np.array([0, 1, 0xFFFFFFFF, 0x80000000, 12345, 0xDEADBEEF], U)
    rr.pin_next_rand(pinned)
    for states in (pinned, np.random.default_rng(1).integers(0, 2**32, 4096, dtype=np.uint64).astype(U)):
        assert np.array_equal(ur.prev_state(rr.next_rand(states)[0]), states)
        assert np.array_equal(rr.next_rand(ur.prev_state(states))[0], states)
    assert (1664525 * ur.LCG_INV) % 2**32 == 1


def test_the_offset_rule_and_the_forked_seed():
    """drawn offsets stay within the radius and the frame, never name the pixel itself, and take two draws a slot; the seed is
    the fork idiom initRand(initRand(pixel, frame), key)"""
    from hlsl_integrator_numpy import hm_init_rand
    W, H, K, R = 13, 7, 5, 3
    seeds = ur.fork_seeds(np.arange(W * H), 9)
    assert seeds[5] == hm_init_rand(hm_init_rand(5, 9), 0x52455553) and len(set(seeds.tolist())) == W * H
    nbr, after = ur.drawn_neighbors(seeds, W, H, K, R)
    s = seeds
    for _ in range(2 * K):
        s = rr.next_rand(s)[0]
    assert np.array_equal(after, s)
    pix = np.arange(W * H)[:, None]
    ok = nbr != ur.NONE
    dx, dy = nbr.astype(np.int64) % W - pix % W, nbr.astype(np.int64) // W - pix // W
    assert ok.any() and (~ok).any() and (nbr[ok] < W * H).all() and (nbr != pix)[ok].all()
    assert (np.abs(dx)[ok] <= R).all() and (np.abs(dy)[ok] <= R).all() and (np.abs(dx)[ok] == R).any()


# ---- the estimator over the CPU oracle -------------------------------------------------------------------------------------
M1, NEIGHBORS = 2, 2  # the first stage's candidates, and the neighbours of the reuse


class _Case:
    def __init__(self, pkg, ob):
        self.lib = ob.load_oracle(pkg.abi)
        self.sc = dr.three_light_scene(pkg)
        self.osc = self.lib.oracle_scene_create(C.byref(self.sc.desc))
        assert self.osc
        self.L = len(self.sc.lights)
        self.backend = rr.OracleBackend(ob, pkg.abi, self.lib, self.osc, self.sc.lights, 1, MIN_T)
        # a state whose next draw chooses light l, for every l
        self.state_of = {}
        s = np.arange(4096, dtype=U)
        _, r = rr.next_rand(s)
        pick = np.minimum((r * F(self.L)).astype(F).astype(np.int64), self.L - 1)
        for l in range(self.L):
            self.state_of[l] = U(s[np.argmax(pick == l)])

    def table(self, rec):
        """v_x(l) (n, L, 3) float32: the clamped value of light l at every record, as the first stage sees it"""
        v = np.zeros((len(rec), self.L, 3), F)
        for l in range(self.L):
            _, value, light, _, _ = self.backend.candidates(rec, np.full(len(rec), self.state_of[l], U))
            assert (light == l).all()
            v[:, l] = rr.clamp_vec(value, rr.FLT_MAX)
        return v

    def close(self):
        self.lib.oracle_scene_destroy(self.osc)


@pytest.fixture(scope="module")
def case(pkg, ob):
    c = _Case(pkg, ob)
    yield c
    c.close()


def _first_stage(t, M):
    """the outcomes (light or -1, W, probability) of M candidates drawn uniformly from the lights with targets t, merged"""
    L = len(t)
    out = {}
    for seq in itertools.product(range(L), repeat=M):
        p = 1.0 / L ** M
        w = [t[l] for l in seq]
        wsum = sum(w)
        if wsum == 0.0:
            out[(-1, 0.0)] = out.get((-1, 0.0), 0.0) + p
            continue
        # sequential reservoir: candidate c survives with probability w_c / wsum
        for c in range(M):
            if w[c] > 0.0:
                key = (seq[c], (wsum / M) / w[c])
                out[key] = out.get(key, 0.0) + p * w[c] / wsum
    return [(l, W, p) for (l, W), p in out.items()]


def _enumerate(v, M, z_is_mtot=False):
    """E[term] and the largest outcome of the reuse of sources v (1 + neighbours, L, 3) float64 — source 0 is the item — each
    holding the reservoir of a first stage with M candidates at its own surface: every candidate sequence, selections with
    probability w / wsum"""
    t = v.max(axis=2)
    outs = [_first_stage(t[j].tolist(), M) for j in range(len(v))]
    E, top = np.zeros(3), 0.0
    for combo in itertools.product(*outs):
        p = math.prod(c[2] for c in combo)
        w = [t[0, l] * W * M if l >= 0 else 0.0 for l, W, _ in combo]
        wsum = sum(w)
        if wsum == 0.0:
            continue
        for j, (l, _, _) in enumerate(combo):
            if w[j] > 0.0:
                Z = M * len(v) if z_is_mtot else sum(M for k in range(len(v)) if t[k, l] > 0.0)
                est = v[0, l] * ((wsum / Z) / t[0, l])
                E += p * (w[j] / wsum) * est
                top = max(top, float(est.max()))
    return E, top


def test_the_estimator_is_unbiased_exactly(pkg, ob, case):
    """(1) three lights, Lambertian, first stage M = 2, two neighbours that are arbitrary other records (no rejection), 64
    items: the float64 enumeration of E[term] over the fp32 per-light values equals sum_l v_i(l) / L to a relative 1e-9 (the
    identity is algebraic; float64 rounding over ~1e4 terms is orders below).  Some source has t_j(l) == 0 < t_i(l) — where 1 / Z
    and 1 / Mtot differ — and the same enumeration with Z = Mtot misses by more than 1e-3 on some item."""
    rng = np.random.default_rng(7)
    n = 64
    rec = case.sc.records(rng, 3 * n)
    v = case.table(rec).astype(np.float64).reshape(n, 3, case.L, 3)  # item k: records 3k (own), 3k + 1 and 3k + 2 (neighbours)
    t = v.max(axis=3)
    assert ((t[:, 1:, :] == 0) & (t[:, 0:1, :] > 0)).any(), "no source is blind to a light the item sees"
    worst, worst_mtot = 0.0, 0.0
    for k in range(n):
        truth = v[k, 0].sum(axis=0) / case.L
        if truth.max() == 0.0:
            continue
        E, _ = _enumerate(v[k], M1)
        worst = max(worst, float(np.abs(E - truth).max() / truth.max()))
        E2, _ = _enumerate(v[k], M1, z_is_mtot=True)
        worst_mtot = max(worst_mtot, float(np.abs(E2 - truth).max() / truth.max()))
    print(f"1 / Z: worst relative deviation {worst:.3e}; with Z = Mtot {worst_mtot:.3e}")
    assert worst <= 1e-9
    assert worst_mtot > 1e-3, "the enumeration cannot see a wrong Z"


ITEMS, PER_ITEM, DELTA = 48, 1024, 1e-9


def test_the_definition_converges_to_the_enumeration(pkg, ob, case):
    """(2) reuse_compose over the oracle (fp32) against the enumeration: 48 items, two neighbours on the item's own plane with
    the rejection tests on (normalMin 0.9, planeMax 1e-3), 1024 independent seeds each for the first stage of every source and
    for the reuse.  A single term lies in [0, R_i], R_i the enumeration's largest outcome.  Hoeffding: |sum_i (mean_s term -
    E_i)| > sqrt(ln(2 / delta) / 2 * sum_i R_i^2 / S) with probability at most delta = 1e-9 per channel.  The bound, the
    deviations and the channel sums are printed; DESIGN.md "Reservoir reuse" records them."""
    rng = np.random.default_rng(2025)
    pool = case.sc.records(rng, 4000)
    N, P = pool[:, 4:7], pool[:, 0:3]
    groups = []
    for i in range(len(pool)):
        same = (ur.dot3(np.repeat(N[i:i + 1], len(pool), 0), N) >= F(0.9)) & \
               (np.abs(ur.dot3(np.repeat(N[i:i + 1], len(pool), 0), (P - P[i]).astype(F))) <= F(1e-3))
        same[i] = False
        j = np.nonzero(same)[0]
        if len(j) >= NEIGHBORS:
            groups.append([i] + rng.choice(j, NEIGHBORS, replace=False).tolist())
        if len(groups) == ITEMS:
            break
    assert len(groups) == ITEMS
    g = np.array(groups)
    base = pool[g.reshape(-1)]  # (ITEMS * 3, 24): own, neighbour, neighbour
    v = case.table(base).astype(np.float64).reshape(ITEMS, 1 + NEIGHBORS, case.L, 3)
    want, R = np.zeros((ITEMS, 3)), np.zeros(ITEMS)
    for k in range(ITEMS):
        want[k], R[k] = _enumerate(v[k], M1)
    bound = math.sqrt(math.log(2.0 / DELTA) / 2.0 * float((R * R).sum()) / PER_ITEM)
    big = np.tile(base, (PER_ITEM, 1))  # repetition r: rows r * ITEMS * 3 ...
    first = rr.ris_compose(case.backend, big, rng.integers(0, 2**32, len(big), dtype=np.uint64).astype(U), M1, 1, min_t=MIN_T)
    res = first["reservoirs"][:, 0, :]
    own = np.arange(0, len(big), 1 + NEIGHBORS)
    nbr = np.stack([own + 1 + k for k in range(NEIGHBORS)], axis=1).astype(U)
    got = ur.reuse_compose(case.backend, big[own], rng.integers(0, 2**32, len(own), dtype=np.uint64).astype(U), res[own], case.L,
                           neighbor_index=nbr, pool_rec=big, pool_res=res, in_m=M1, pool_m=M1, normal_min=0.9, plane_max=1e-3)
    assert (got["skipped"] == 0).all() and (got["source"] > 0).any() and (got["source"] == 0).any()
    terms = got["terms"].astype(np.float64).reshape(PER_ITEM, ITEMS, 3)
    assert (terms.max(axis=2).max(axis=0) <= R * (1 + 1e-5)).all(), "a single term exceeds its enumerated range"
    dev = np.abs((terms.mean(axis=0) - want).sum(axis=0))
    total = want.sum(axis=0)
    print(f"bound {bound:.4f}, deviation {dev[0]:.4f} {dev[1]:.4f} {dev[2]:.4f}, sum E {total[0]:.3f} {total[1]:.3f} {total[2]:.3f}"
          f" ({100 * bound / total.min():.2f} % of the smallest)")
    assert (dev <= bound).all(), (bound, dev)
    assert bound < 0.25 * total.min(), "the bound is too loose to see a wrong Z or W"


# ---- the pipeline's history and the host pass ------------------------------------------------------------------------------
def test_every_scene_change_drops_the_restir_history(pkg):
    """set_lights, update_geometry, update_skinned, update_morphed, set_skin and set_morph each make the next restir_lighting
    call start without a history: its samples would be re-evaluated against other lights or surfaces"""
    import torch

    class Ctx:
        def __getattr__(self, name):
            return lambda *a, **k: None

    pipe = pkg.FramePipeline.__new__(pkg.FramePipeline)
    pipe.ctx, pipe.torch, pipe.dev, pipe.accum_count = Ctx(), torch, torch.device("cpu"), 5
    pipe._stream_ptr = lambda: None
    pipe._restir = None
    pipe.set_lights([])  # no history yet: nothing to drop
    calls = (lambda: pipe.set_lights([]), lambda: pipe.update_geometry(None), lambda: pipe.update_skinned(None), lambda: pipe.update_morphed(None),
             lambda: pipe.set_skin(None, None, None, 1), lambda: pipe.set_morph(None, None, None))
    real = pkg.keep_for_stream
    pkg.keep_for_stream = lambda stream, tensors: None
    orig_stream = torch.cuda.current_stream
    torch.cuda.current_stream = lambda dev=None: None
    try:
        for call in calls:
            pipe._restir = dict(valid=True)
            call()
            assert pipe._restir["valid"] is False
    finally:
        pkg.keep_for_stream, torch.cuda.current_stream = real, orig_stream


def test_bdpt_render_parses_and_refuses_reuse_options():
    """the reuse switches without --ris M, N, R and C outside their ranges, --ris-radius or --ris-max-m without what they go
    with, and reuse with several samples, hints, frames in flight or a moving scene exit with status 2 and a message, before any
    GPU is touched; the usage names the options and the pass has its reference-style name and setters"""
    import subprocess
    host = os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "host")
    assert "using bdpt::RestirDirectPass;" in open(os.path.join(host, "ReferenceNames.h")).read()
    head = open(os.path.join(host, "Passes.h")).read().split("class RestirDirectPass")[1].split("};")[0]
    for setter in ("setCandidates", "setSpatial", "setRadius", "setTemporal", "setMaxM", "setMaterial", "setAreaLights", "setClamp"):
        assert f"void {setter}(" in head, setter
    assert "holdsTemporalState() override { return true; }" in head and "saveState(" in head and "loadState(" in head
    render = os.path.join(host, "bdpt_render")
    if not os.path.exists(render):
        pytest.skip("host/bdpt_render not built")
    goes, needs = "go with --ris M", "--ris-spatial N needs N in 0 .. 8"
    for args, text in ((["--ris-spatial", "2"], goes), (["--ris-temporal"], goes), (["--ris-radius", "4"], goes), (["--ris-max-m", "40"], goes),
                       (["--ris", "4", "--ris-spatial", "9"], needs), (["--ris", "4", "--ris-spatial", "-1"], needs),
                       (["--ris", "4", "--ris-radius", "4"], needs), (["--ris", "4", "--ris-spatial", "2", "--ris-radius", "0"], needs),
                       (["--ris", "4", "--ris-spatial", "2", "--ris-radius", "1025"], needs), (["--ris", "4", "--ris-max-m", "40"], needs),
                       (["--ris", "4", "--ris-temporal", "--ris-max-m", "0"], needs), (["--ris", "4", "--ris-temporal", "--ris-samples", "2"], needs),
                       (["--ris", "4", "--ris-spatial", "2", "--ris-hints"], needs), (["--ris", "4", "--ris-temporal", "--inflight", "2"], needs),
                       (["--ris", "4", "--ris-temporal", "--sway", "0.1"], needs), (["--ris", "4", "--ris-spatial", "1", "--bend", "0.1"], needs),
                       (["--ris", "4", "--ris-temporal", "--gpus", "1"], "--ris M needs M in 1 .. 32"),
                       (["--ris", "4", "--ris-temporal", "--denoise"], "not with")):
        r = subprocess.run([render] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and text in r.stderr, (args, r.stderr)
    u = subprocess.run([render, "--help"], capture_output=True, text=True, timeout=60)
    assert "[--ris-spatial N [--ris-radius R]] [--ris-temporal] [--ris-max-m C]" in u.stderr
