"""Yardsticks of reservoir reuse (bdpt_reuse_query and bdpt_reuse_execute, include/bdpt.h "Reservoir reuse"), none of them the
code under test.

reuse_compose is the query's definition written once in numpy float32, one operation per rounding, over the backend protocol
of ris_reference.ris_compose: its evaluation step is backend.candidates(rec, prev(state)) — ONE next-event sample per record
from the state before the selection draw, which draws the record's light again — so ris_reference.OracleBackend and the
composed device loop of tests/test_gpu_ris.py serve it unchanged; any_hit(rays) settles the survivor.  drawn_neighbors is the
execute call's offset rule and fork_seeds its seeds."""
import numpy as np

import ris_reference as rr
from hlsl_integrator_numpy import hm_init_rand

F, U = np.float32, np.uint32
NO_LIGHT, STATUS_RAY, STATUS_OCCLUDED = rr.NO_LIGHT, rr.STATUS_RAY, rr.STATUS_OCCLUDED
MAX_NEIGHBORS, MAX_M = 8, 1 << 24
NONE = 0xFFFFFFFF
STREAM_KEY = 0x52455553
LCG_INV = 4276115653  # 1664525 * LCG_INV == 1 mod 2^32


def prev_state(states):
    """the generator's inverse: prev(next(s)) == s"""
    s = np.asarray(states, U).astype(np.uint64)
    return (((s + np.uint64(2**32 - 1013904223)) & np.uint64(0xFFFFFFFF)) * np.uint64(LCG_INV) & np.uint64(0xFFFFFFFF)).astype(U)


def dot3(a, b):
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).astype(F) + a[:, 2] * b[:, 2]).astype(F)


def _count(scalar, word):
    m = np.full(len(word), scalar, U) if scalar else word.astype(U)
    return np.minimum(m, U(MAX_M))


def evaluate(backend, rec, y, lights_count, clamp):
    """v_x(y), t_x(y) of records y (m, 4) uint32 at surfaces rec (m, 24) -> (v (m, 3), t (m,), ray (m, 8), empty (m,) bool)"""
    m = len(rec)
    light, W = y[:, 0] & U(0xFFFF), y[:, 2].copy().view(F)
    with np.errstate(all="ignore"):
        full = (light < U(lights_count)) & (light != U(NO_LIGHT)) & (W > 0)
    v, ray = np.zeros((m, 3), F), np.zeros((m, 8), F)
    j = np.nonzero(full)[0]
    if len(j):
        r, value, got_light, _, after = backend.candidates(np.ascontiguousarray(rec[j]), prev_state(y[j, 1]))
        assert np.array_equal(after, y[j, 1]), "prev(state) then one draw is the record's state"
        assert np.array_equal(got_light.astype(U), light[j]), "prev(state) draws the record's light"
        v[j], ray[j] = rr.clamp_vec(value, clamp), r
    return v, rr.maxf(rr.maxf(v[:, 0], v[:, 1]), v[:, 2]), ray, ~full


def reuse_compose(backend, rec, seeds, res_in, lights_count, neighbor_index=None, pool_rec=None, pool_res=None, pool_alive=None, in_m=0,
                  pool_m=0, max_m=MAX_M, normal_min=-np.inf, plane_max=np.inf, clamp=rr.FLT_MAX, alive=None):
    """bdpt_reuse_query's definition over `backend` on (n, 24) bdpt_surface records, (n,) uint32 states and (n, 4) uint32 own
    records; the pool defaults to the items.  -> dict(color (n, 4), seeds_out, traced, out (n, 4) uint32, live (n,) bool,
    skipped (n,) slots skipped, source (n,) int: the selected source (0 own, 1 .. neighbours, -1 none), empty (n,) sources
    with an empty record, terms (n, 3) the term before visibility)"""
    rec = np.ascontiguousarray(rec, F)
    res_in = np.ascontiguousarray(res_in).view(U).reshape(-1, 4)
    n = len(rec)
    live = rec.view(np.int32)[:, 23] >= 0
    if alive is not None:
        live = live & (np.asarray(alive) != 0)
    nbr = np.zeros((n, 0), U) if neighbor_index is None else np.ascontiguousarray(neighbor_index).view(U).reshape(n, -1)
    K = nbr.shape[1]
    assert K <= MAX_NEIGHBORS
    if pool_rec is None:
        pool_rec, pool_res, pool_alive = rec, res_in, alive
    pool_rec = np.ascontiguousarray(pool_rec, F)
    pool_res = np.ascontiguousarray(pool_res).view(U).reshape(-1, 4)
    P = len(pool_rec)
    pool_live = pool_rec.view(np.int32)[:, 23] >= 0
    if pool_alive is not None:
        pool_live = pool_live & (np.asarray(pool_alive) != 0)
    idx = np.nonzero(live)[0]
    sub = np.ascontiguousarray(rec[idx])
    m = len(idx)
    s = np.ascontiguousarray(seeds, U)[idx].copy()
    wsum, mtot = np.zeros(m, F), np.zeros(m, U)
    sel = np.zeros(m, bool)
    v_sel, t_sel, ray_sel = np.zeros((m, 3), F), np.zeros(m, F), np.zeros((m, 8), F)
    y_sel, source = np.zeros((m, 4), U), np.full(m, -1, np.int64)
    skipped, empties = np.zeros(m, np.int64), np.zeros(m, np.int64)
    kept = []  # per neighbour slot: (ok, pool index, count)
    with np.errstate(all="ignore"):
        for j in range(K + 1):
            s, u = rr.next_rand(s)
            if j == 0:
                ok, y, cnt = np.ones(m, bool), res_in[idx], _count(in_m, res_in[idx, 3])
            else:
                p = nbr[idx, j - 1]
                ok = p < U(P)
                q = np.where(ok, p, U(0)).astype(np.int64) if P else np.zeros(m, np.int64)
                if P:
                    ok &= pool_live[q]
                    ok &= dot3(sub[:, 4:7], pool_rec[q, 4:7]) >= F(normal_min)
                    ok &= np.abs(dot3(sub[:, 4:7], (pool_rec[q, 0:3] - sub[:, 0:3]).astype(F))) <= F(plane_max)
                    y, cnt = pool_res[q], np.minimum(_count(pool_m, pool_res[q, 3]), U(max_m))
                else:
                    y, cnt = np.zeros((m, 4), U), np.zeros(m, U)
                kept.append((ok, q, cnt))
                skipped += ~ok
            v, t, ray, none = np.zeros((m, 3), F), np.zeros(m, F), np.zeros((m, 8), F), np.ones(m, bool)
            k = np.nonzero(ok)[0]
            if len(k):
                v[k], t[k], ray[k], none[k] = evaluate(backend, sub[k], y[k], lights_count, clamp)
                empties[k] += none[k]
            w = ((t * y[:, 2].copy().view(F)).astype(F) * cnt.astype(F)).astype(F)
            w[none] = F(0)  # an empty record: w = 0, whatever its W is
            wsum = np.where(ok, (wsum + w).astype(F), wsum)
            mtot = np.where(ok, mtot + cnt, mtot).astype(U)
            take = ok & (w > 0) & ((u * wsum).astype(F) <= w)
            sel |= take
            v_sel[take], t_sel[take], ray_sel[take], y_sel[take], source[take] = v[take], t[take], ray[take], y[take], j
        Z = np.where(sel & (t_sel > 0), _count(in_m, res_in[idx, 3]), U(0)).astype(U)
        for ok, q, cnt in kept:
            k = np.nonzero(sel & ok)[0]
            if len(k):
                _, t, _, _ = evaluate(backend, np.ascontiguousarray(pool_rec[q[k]]), y_sel[k], lights_count, clamp)
                Z[k] += np.where(t > 0, cnt[k], U(0)).astype(U)
        sel &= Z != 0
        source[~sel] = -1
        W = ((wsum / Z.astype(F)).astype(F) / t_sel).astype(F)
        term = (v_sel * W[:, None]).astype(F)
    occluded = np.zeros(m, bool)
    if sel.any():
        k = np.nonzero(sel)[0]
        occluded[k] = ~np.asarray(backend.any_hit(np.ascontiguousarray(ray_sel[k])), bool)
    status = np.where(sel, U(STATUS_RAY), U(0)) | np.where(occluded, U(STATUS_OCCLUDED), U(0))
    out = np.zeros((m, 4), U)
    out[:, 0] = np.where(sel, (y_sel[:, 0] & U(0xFFFF)) | (status << U(16)), U(NO_LIGHT))
    out[:, 1] = np.where(sel, y_sel[:, 1], U(0))
    out[:, 2] = np.where(sel, W, F(0)).astype(F).view(U)
    out[:, 3] = mtot
    color = np.concatenate([rec[:, 12:15], np.ones((n, 1), F)], axis=1).astype(F)
    color[idx, 0:3] = np.where((sel & ~occluded)[:, None], term, F(0))
    seeds_out = np.ascontiguousarray(seeds, U).copy()
    seeds_out[idx] = s
    full = lambda a, fill=0: _scatter(n, idx, a, fill)  # noqa: E731
    all_out = np.zeros((n, 4), U)
    all_out[:, 0] = NO_LIGHT
    all_out[idx] = out
    terms = np.zeros((n, 3), F)
    terms[idx] = np.where(sel[:, None], term, F(0))
    return dict(color=color, seeds_out=seeds_out, traced=full(sel.astype(U)), out=all_out, live=live, skipped=full(skipped),
                source=full(source, -1), empty=full(empties), terms=terms)


def _scatter(n, idx, a, fill):
    r = np.full(n, fill, a.dtype)
    r[idx] = a
    return r


def fork_seeds(pixels, frame_count):
    """the execute call's seeds: initRand(initRand(pixel, frameCount), 0x52455553)"""
    return np.array([hm_init_rand(hm_init_rand(int(p), int(frame_count)), STREAM_KEY) for p in pixels], U)


def drawn_neighbors(seeds, width, height, neighbors, radius):
    """the execute call's drawn offsets for every pixel of the frame, in pixel order: per slot u1, u2, dx = (int)(u1 * (float)(2 *
    radius + 1)) - radius, dy likewise; none when (dx, dy) == (0, 0) or outside the frame -> (index (W * H, neighbors) uint32, the
    states after the 2 * neighbors draws)"""
    s = np.ascontiguousarray(seeds, U).copy()
    n = width * height
    assert len(s) == n
    x, y = np.arange(n) % width, np.arange(n) // width
    side = F(2 * radius + 1)
    out = np.full((n, neighbors), NONE, U)
    for k in range(neighbors):
        s, u1 = rr.next_rand(s)
        s, u2 = rr.next_rand(s)
        dx = (u1 * side).astype(F).astype(np.int64) - radius
        dy = (u2 * side).astype(F).astype(np.int64) - radius
        nx, ny = x + dx, y + dy
        ok = ((dx != 0) | (dy != 0)) & (nx >= 0) & (ny >= 0) & (nx < width) & (ny < height)
        out[ok, k] = (ny * width + nx)[ok].astype(U)
    return out, s
