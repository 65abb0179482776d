"""Yardsticks of resampled direct lighting (bdpt_ris_query, include/bdpt.h "Resampled direct lighting"), none of them the code
under test.

ris_compose is the query's definition written once in numpy float32, one operation per rounding, over a small backend:
candidates(rec, states) -> (ray (n, 8), value (n, 3), light (n,), status (n,), states_out (n,)) is ONE next-event sample per
record and state, in bdpt_light_query's terms; any_hit(rays) -> unoccluded (n,) bool; hint_occluded(rec, states) -> (n,) bool is
bdpt_light_query's hint bit for the candidate drawn from `states`.  OracleBackend takes candidates from oracle_light_nee and
visibility from oracle_trace mode 2 (the oracle has no occluder hints: it serves hints=False); the emitter table's candidates
come from oracle_area_light_sample mode 1 and the Lambertian restatement tests/test_gpu_light_queries.py checks against.  tests/test_gpu_ris.py answers
the same backend with Context.sample_lights(..., seeds_out=...) and Context.trace_rays(..., "any"): the composed loop."""
import numpy as np

import direct_reference as dr
import hlsl_reference_math as hm

F, U = np.float32, np.uint32
FLT_MAX = float(np.finfo(np.float32).max)
NO_LIGHT = 0xFFFF
STATUS_RAY, STATUS_HINT_OCCLUDED, STATUS_OCCLUDED = 1, 2, 4
USE_HINTS = 1


def next_rand(states):
    """hlsl_reference_math.next_rand for an array of states -> (states after, draws float32); tests/test_ris_cpu.py pins the two"""
    s = ((np.asarray(states, np.uint64) * np.uint64(1664525) + np.uint64(1013904223)) & np.uint64(0xFFFFFFFF)).astype(U)
    return s, ((s & U(0x00FFFFFF)).astype(F) / F(0x01000000)).astype(F)


def clamp_vec(v, hi):
    """clampVec: NaN and negative components become +0, then the upper bound"""
    y = np.where(v > 0, v, F(0)).astype(F)
    return np.where(y < F(hi), y, F(hi)).astype(F)


def maxf(a, b):
    return np.where(b > a, b, a).astype(F)


def with_view(rec, rng):
    """records given what the GGX material reads besides N and the colours: a unit V on N's side (words 8-10) and a
    linearRoughness in 0.15 .. 0.9 (word 7); every ninth V points below the surface (NdotV = 0: the value is NaN)"""
    rec = rec.copy()
    n = len(rec)
    d = rng.normal(size=(n, 3))
    v = rec[:, 4:7].astype(np.float64) + 0.8 * d / np.linalg.norm(d, axis=1, keepdims=True)
    v[::9] = -rec[::9, 4:7]
    with np.errstate(all="ignore"):
        rec[:, 8:11] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
    rec[:, 7] = rng.uniform(0.15, 0.9, n).astype(F)
    return rec


def ris_compose(backend, rec, seeds, M, K, clamp=FLT_MAX, min_t=1e-4, hints=False, alive=None):
    """bdpt_ris_query's definition over `backend` on (n, 24) bdpt_surface records and (n,) uint32 states.
    -> dict(color (n, 4) float32, seeds_out (n,) uint32, traced (n,) uint32, reservoirs (n, K, 4) uint32, live (n,) bool,
    terms (K, n, 3) float32: the terms before visibility, selected (K, n) int: the selected light or -1)"""
    rec = np.ascontiguousarray(rec, F)
    n = len(rec)
    live = rec.view(np.int32)[:, 23] >= 0
    if alive is not None:
        live = live & (np.asarray(alive) != 0)
    idx = np.nonzero(live)[0]
    sub = np.ascontiguousarray(rec[idx])
    m = len(idx)
    s = np.ascontiguousarray(seeds, U)[idx].copy()
    total = np.zeros((m, 3), F)
    traced = np.zeros(m, U)
    res = np.zeros((m, K, 4), U)
    terms, selected = np.zeros((K, n, 3), F), np.full((K, n), -1, np.int64)
    with np.errstate(all="ignore"):
        for k in range(K):
            wsum = np.zeros(m, F)
            sel = np.zeros(m, bool)
            v_sel, w_sel = np.zeros((m, 3), F), np.zeros(m, F)
            ray_sel, light_sel = np.zeros((m, 8), F), np.zeros(m, U)
            state_sel, before_sel = np.zeros(m, U), np.zeros(m, U)
            for _ in range(M):
                before = s.copy()
                ray, value, light, _, s_after = backend.candidates(sub, before)
                assert np.array_equal(s_after, next_rand(before)[0]), "a candidate takes exactly one draw"
                s, u = next_rand(s_after)
                v = clamp_vec(value, clamp)
                w = maxf(maxf(v[:, 0], v[:, 1]), v[:, 2])
                wsum = (wsum + w).astype(F)
                take = (w > 0) & ((u * wsum).astype(F) <= w)
                sel |= take
                v_sel[take], w_sel[take], ray_sel[take], light_sel[take] = v[take], w[take], ray[take], light[take]
                state_sel[take], before_sel[take] = s_after[take], before[take]
            W = ((wsum / F(M)).astype(F) / w_sel).astype(F)
            term = (v_sel * W[:, None]).astype(F)
            status = np.where(sel, U(STATUS_RAY), U(0))
            need = sel.copy()
            if hints and sel.any():
                positive = (term > 0).any(axis=1)
                ask = np.nonzero(sel & positive)[0]
                if len(ask):
                    hinted = np.zeros(m, bool)
                    hinted[ask] = backend.hint_occluded(np.ascontiguousarray(sub[ask]), before_sel[ask])
                    status[hinted] |= U(STATUS_HINT_OCCLUDED)
                    need &= ~hinted
            occluded = np.zeros(m, bool)
            if need.any():
                j = np.nonzero(need)[0]
                occluded[j] = ~np.asarray(backend.any_hit(np.ascontiguousarray(ray_sel[j])), bool)
            status[occluded] |= U(STATUS_OCCLUDED)
            traced += need.astype(U)
            add = sel & ((status & U(STATUS_HINT_OCCLUDED | STATUS_OCCLUDED)) == 0)
            total = np.where(add[:, None], total + term, total).astype(F)
            res[:, k, 0] = np.where(sel, light_sel | (status << U(16)), U(NO_LIGHT))
            res[:, k, 1] = np.where(sel, state_sel, U(0))
            res[:, k, 2] = np.where(sel, W, F(0)).astype(F).view(U)
            res[:, k, 3] = wsum.view(U)
            terms[k, idx] = np.where(sel[:, None], term, F(0))
            selected[k, idx] = np.where(sel, light_sel.astype(np.int64), -1)
        color = (total / F(K)).astype(F)
    out_color = np.concatenate([rec[:, 12:15], np.ones((n, 1), F)], axis=1).astype(F)
    out_color[idx, 0:3] = color
    seeds_out = np.ascontiguousarray(seeds, U).copy()
    seeds_out[idx] = s
    all_traced = np.zeros(n, U)
    all_traced[idx] = traced
    all_res = np.zeros((n, K, 4), U)
    all_res[:, :, 0] = NO_LIGHT
    all_res[idx] = res
    return dict(color=out_color, seeds_out=seeds_out, traced=all_traced, reservoirs=all_res, live=live, terms=terms, selected=selected)


def lambert_value(lights_count, L, intensity, N, dif):
    """directIfVisible of the Lambertian material in its operation order (the restatement tests/test_gpu_light_queries.py
    checks bdpt_light_query's table samples against)"""
    d = (N[:, 0] * L[:, 0] + N[:, 1] * L[:, 1]) + N[:, 2] * L[:, 2]
    y = np.where(d > 0, d, F(0))
    ldn = np.where(y < 1, y, F(1)).astype(F)
    return ((((F(lights_count) * ldn)[:, None] * intensity) * dif) / F(3.14159265358979323846)).astype(F)


class OracleBackend:
    """ris_compose's backend from the CPU oracle's hooks (no hints).  area=True: the emitter table is light numLights of
    numLights + 1 while the oracle's table has weight, Lambertian only: oracle_light_nee runs on the lights plus one stand-in
    entry, so that its light count and choice are the pass's, and the items that chose the stand-in take the table's
    candidate from oracle_area_light_sample mode 1 (L, distance, intensity at the state after the selection draw) through
    lambert_value, with the (1 - 1e-4) distance."""

    def __init__(self, ob, abi, lib, osc, lights, mat_index, min_t, area=False):
        import ctypes as C
        self.ob, self.abi, self.lib, self.osc, self.mat, self.min_t = ob, abi, lib, osc, mat_index, min_t
        self.num_lights = len(lights)
        self.table = False
        if area:
            assert mat_index == 1, "the table's value is restated for the Lambertian material only"
            info = abi.AreaLightInfo()
            lib.oracle_area_light_info(osc, C.byref(info))
            self.table = info.numEmitters > 0 and info.totalWeight > 0
        if self.table:
            ext = (abi.Light * (self.num_lights + 1))()
            for k in range(self.num_lights + 1):
                C.memmove(C.byref(ext[k]), C.byref(lights[min(k, self.num_lights - 1)]), C.sizeof(abi.Light))
            lights = ext
        self.lights = lights
        self._trace = dr.OracleBackend(ob, abi, lib, osc, lights, min_t)

    def candidates(self, rec, states):
        smp, after = self.ob.light_nee(self.abi, self.lights, rec, states, self.mat, self.min_t)
        smp = smp.copy()
        word = smp.view(U)[:, 11]
        if self.table:
            from area_scenes import oracle_sample
            j = np.nonzero((word & U(0xFFFF)) == U(self.num_lights))[0]
            if len(j):
                pts = np.ascontiguousarray(rec[j, 0:3])
                ref = oracle_sample(self.lib, self.osc, 1, after[j], pts)
                with np.errstate(all="ignore"):
                    value = lambert_value(self.num_lights + 1, ref[:, 1:4], ref[:, 5:8], rec[j, 4:7], rec[j, 12:15])
                    smp[j, 4:7], smp[j, 7] = ref[:, 1:4], (ref[:, 4] * (F(1.0) - F(1e-4))).astype(F)
                smp[j, 8:11] = value
                word[j] = U(self.num_lights) | ((value != 0).any(axis=1).astype(U) << U(16))
        return smp[:, 0:8].copy(), smp[:, 8:11].copy(), word & U(0xFFFF), word >> U(16), after

    def any_hit(self, rays):
        return self._trace.any_hit(rays)

    def hint_occluded(self, rec, states):
        raise NotImplementedError("the oracle has no occluder hints")


def pin_next_rand(states):
    """next_rand above against hlsl_reference_math.next_rand, one state at a time"""
    after, draws = next_rand(states)
    for s0, s1, r in zip(np.asarray(states, U).tolist(), after.tolist(), draws.tolist()):
        want_s, want_r = hm.next_rand(s0)
        assert (s1, r) == (want_s, float(F(want_r))), (s0, s1, r)
