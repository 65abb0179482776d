"""GPU tests of what the four persistent query kernels share (csrc/device_item_loop.hpp): the fetch from the context's one
cursor and its release.  bdpt_ao_query, bdpt_gi_query and bdpt_walk_query through whole chunks of dead items, against the
composed loops of their own tests, and all four kernels back to back on one stream.  Every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library is loaded, as test_gpu_gi.py explains)

import gi_reference as gr
import test_gpu_ao as ga
import test_gpu_gi as gg
import test_gpu_walk_query as gw
from walk_loop import ContextQueries, gpu, host, walk_loop

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
MIN_T = ga.MIN_T
AO_S, WALK_STEPS = 2, 2


def _live_items(s, n):
    """n of the Cornell state's records that hit the scene, spread over the image, with their seeds"""
    live = np.nonzero(s["surf"].view(np.int32)[:, 23] >= 0)[0]
    pick = live[np.linspace(0, len(live) - 1, n).astype(np.int64)]
    return s["surf"][pick].copy(), s["seeds"][pick].copy()


def _walk_starts(surf):
    """walk starts that leave the records' positions along their normals, with a colour per item"""
    n = len(surf)
    starts = np.zeros((n, 12), F)
    starts[:, 0:3], starts[:, 3], starts[:, 4:7], starts[:, 7] = surf[:, 0:3], F(MIN_T), surf[:, 4:7], F(1e38)
    starts[:, 8:11] = np.random.default_rng(41).uniform(0.1, 1.0, (n, 3)).astype(F)
    return starts


def _walk(ctx, starts, seeds, alive):
    return gw._run(lambda *a, **kw: ctx.walk(*a, mat_index=0, min_t=MIN_T, **kw), starts, seeds.view(np.int32), WALK_STEPS, alive=alive)


@pytest.mark.parametrize("n,dead", [(200, 128), (130, 130)])
def test_runs_of_dead_items(pkg, ob, n, dead):
    """Items whose first `dead` have alive == 0.  The chunk is 64 at these sizes, so waves receive whole chunks without a
    live item: they hold nothing although the list goes on (200 items), or never hold an item at all (130, all dead).
    Outputs equal the composed loops'; a second identical call gives the same bits — the cursor was back at zero."""
    a, g = ga._cornell(pkg, ob), gg._cornell(pkg, ob)
    alive = (np.arange(n) >= dead).astype(np.uint8)
    surf, seeds = _live_items(a, n)
    radius = 0.25 * a["ext"]
    ctx = a["pipe"].ctx
    want = ga.ao_loop(ctx, surf, seeds, AO_S, radius, alive=alive)
    for call in (1, 2):
        got = ga.ao_query(ctx, surf, seeds, AO_S, radius, alive=alive)
        ga._assert_same(got, want, f"ambient_occlusion, call {call}")
        assert (got[0][:dead] == 1.0).all() and (got[1][:dead] == AO_S).all() and np.array_equal(got[2][:dead], seeds[:dead])
    starts = _walk_starts(surf)
    want = walk_loop(ContextQueries(ctx, 0, MIN_T), starts, seeds.view(np.int32), WALK_STEPS, alive=alive)
    for call in (1, 2):
        got = _walk(ctx, starts, seeds, alive)
        gw._assert_equal(got, want, f"walk, call {call}")
        assert (got[1].view(U)[:, :dead, 3] == 0).all() and (got[1].view(U)[0, dead:, 3] != 0).all()
    surf, seeds = _live_items(g, n)
    want = gg.gi_loop(g["ctx"], g["lib"], surf, seeds, gr.INDIRECT, alive=alive)
    for call in (1, 2):
        got = gg.gi_query(g["ctx"], surf, seeds, gr.INDIRECT, alive=alive)
        gg._assert_same(got, want, f"diffuse_gi, call {call}")
        assert np.array_equal(got["seeds_out"][:dead], seeds[:dead]) and (got["status"][:dead] == 0).all()


def test_one_cursor_four_kernels(pkg, ob):
    """A trace (closest, 65 rays), an AO query (65 items, 2 samples), a GI query (65 items, with the bounce), a walk query
    (65 starts, 2 steps) and the trace again, on one stream with no synchronise between them.  Each result equals that of
    the same sequence with a synchronise after every call (whose first call found a fresh cursor), every output word is
    written, and the second trace equals the first: a kernel that left the cursor non-zero would starve the next."""
    a = ga._cornell(pkg, ob)
    ctx, radius, n = a["pipe"].ctx, 0.25 * a["ext"], 65
    surf, seeds = _live_items(a, n)
    starts = _walk_starts(surf)
    rays_t, surf_t, seeds_t, starts_t = gpu(starts[:, 0:8]), gpu(surf), gpu(seeds.view(np.int32)), gpu(starts)

    def outputs():
        f = lambda *shape: torch.full(shape, -7.0, dtype=torch.float32, device="cuda")
        i = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device="cuda")
        return dict(trace1=f(n, 4), ao=f(n), ao_counts=i(n), ao_seeds=i(n), gi=f(n, 4), gi_hits=f(n, 4), gi_status=i(n), gi_seeds=i(n),
                    vertices=f(WALK_STEPS, n, 24), info=f(WALK_STEPS, n, 4), samples=f(WALK_STEPS, n, 8), walk_hits=f(WALK_STEPS, n, 4),
                    trace2=f(n, 4))

    def calls(o, st):
        return [lambda: ctx.trace_rays(rays_t, "closest", out=o["trace1"], stream=st),
                lambda: ctx.ambient_occlusion(surf_t, seeds_t, AO_S, radius, min_t=MIN_T, out=o["ao"], counts=o["ao_counts"],
                                              seeds_out=o["ao_seeds"], stream=st),
                lambda: ctx.diffuse_gi(surf_t, seeds_t, indirect=True, min_t=MIN_T, out=o["gi"], hits=o["gi_hits"], status=o["gi_status"],
                                       seeds_out=o["gi_seeds"], stream=st),
                lambda: ctx.walk(starts_t, seeds_t, WALK_STEPS, min_t=MIN_T, out=(o["vertices"], o["info"]), samples=o["samples"],
                                 hits=o["walk_hits"], stream=st),
                lambda: ctx.trace_rays(rays_t, "closest", out=o["trace2"], stream=st)]

    alone, together = outputs(), outputs()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        st = C.c_void_p(side.cuda_stream)
        for call in calls(alone, st):
            call()
            side.synchronize()
        for call in calls(together, st):
            call()
        side.synchronize()
    for k in alone:
        assert not (host(alone[k]) == -7).any(), k  # written, every word
        assert np.array_equal(host(together[k]).view(U), host(alone[k]).view(U)), k
    assert np.array_equal(host(alone["trace1"]).view(U), host(alone["trace2"]).view(U))
    assert (host(alone["trace1"]).view(np.int32)[:, 3] >= 0).any() and (host(alone["gi_status"]) & gr.BOUNCE_HIT).any()
