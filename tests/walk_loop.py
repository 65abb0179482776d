"""The composed loop bdpt_walk_query replaces, for the walk query's GPU tests (tests/test_gpu_walk_query.py): per bounce
trace_rays("closest") -> shade_hits(normal_map=False) -> sample_bsdf, and between them glue that selects the hits, multiplies
the colours (torch, on the device) and builds the next rays (numpy).  It restates the loop of test_gpu_connect_queries._walk in the terms of
include/bdpt.h "Walk queries": start records, an optional predecessor, one seed per item or per step, planes per step."""
import numpy as np

F = np.float32
STORED, REAL, SPECULAR = 1, 2, 4


def gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def prim_of(rec):
    return rec.view(np.int32)[..., 23]


class PipeQueries:
    """the three queries of a FramePipeline: its BSDF, min_t, SPECULAR_FROM_LOBE flag and stream"""

    def __init__(self, pipe):
        self.pipe, self.min_t = pipe, pipe.min_t

    def trace(self, rays):
        import torch
        hits = torch.empty((rays.shape[0], 4), dtype=torch.float32, device=rays.device)
        self.pipe.trace_rays(rays, "closest", out=hits)
        return hits

    def shade(self, rays, hits):
        return self.pipe.shade_hits(rays, hits, normal_map=False)

    def sample(self, surf, seeds):
        return self.pipe.sample_bsdf(surf, seeds)


class ContextQueries:
    """the same on a bare Context"""

    def __init__(self, ctx, mat_index=0, min_t=1e-4, from_lobe=False):
        self.ctx, self.mat, self.min_t, self.lobe = ctx, mat_index, min_t, from_lobe

    def trace(self, rays):
        import torch
        hits = torch.empty((rays.shape[0], 4), dtype=torch.float32, device=rays.device)
        self.ctx.trace_rays(rays, "closest", out=hits)
        return hits

    def shade(self, rays, hits):
        return self.ctx.shade_hits(rays, hits, normal_map=False)

    def sample(self, surf, seeds):
        return self.ctx.sample_bsdf(surf, seeds, self.mat, self.lobe)


def walk_loop(q, starts, seeds, steps, seed_per_step=False, first=None, first_specular=None, alive=None):
    """starts (N, 12) float32, seeds (N,) or (steps, N) uint32 / int32, first (N, 24), first_specular / alive (N,) uint8: numpy.
    Returns numpy (vertices (steps, N, 24), info (steps, N, 4) float32 with the status bits in column 3, samples
    (steps, N, 8), hits (steps, N, 4)) as bdpt_walk_query defines them."""
    import torch
    n = starts.shape[0]
    starts = np.ascontiguousarray(starts, F)
    payload = np.zeros((n, 24), F)
    payload[:, 0:3] = starts[:, 0:3]
    if first is not None:
        payload = np.ascontiguousarray(first).view(F).copy()
    pspec = np.zeros(n, bool) if first_specular is None else first_specular != 0
    # the colour product runs on the device (torch), so that a NaN weight gives the bits the GPU's multiply gives
    pcolor, L = gpu(starts[:, 8:11]), starts[:, 4:7].copy()
    live = np.ones(n, bool) if alive is None else alive != 0
    seeds = np.ascontiguousarray(seeds).view(np.int32)
    vertices, info = np.zeros((steps, n, 24), F), np.zeros((steps, n, 4), F)
    samples, hits = np.zeros((steps, n, 8), F), np.zeros((steps, n, 4), F)
    for s in range(steps):
        rays = np.zeros((n, 8), F)
        rays[:, 0:3], rays[:, 4:7] = payload[:, 0:3], L
        rays[:, 3] = starts[:, 3] if s == 0 else F(q.min_t)
        rays[:, 7] = starts[:, 7] if s == 0 else F(1e38)
        rays[~live] = 0  # a zero direction: a miss
        rt = gpu(rays)
        ht = q.trace(rt)
        new = q.shade(rt, ht)
        smp_t = q.sample(new, gpu(seeds[s] if seed_per_step else seeds))
        smp, ht, new = host(smp_t), host(ht), host(new)
        hit = live & (prim_of(new) >= 0)
        payload = np.where(hit[:, None], new, payload)
        pspec = np.where(hit, smp.view(np.uint32)[:, 7] != 0, pspec)
        pcolor = torch.where(gpu(hit)[:, None], pcolor * smp_t[:, 4:7], torch.zeros_like(pcolor))
        L = np.where(hit[:, None], smp[:, 0:3], L)
        v = payload.copy()
        prim_of(v)[:] = np.maximum(prim_of(v), 0)
        v[~live] = 0
        prim_of(v)[~live] = -1
        vertices[s] = v
        info[s, :, 0:3] = np.where(live[:, None], host(pcolor), F(0))
        info[s].view(np.uint32)[:, 3] = np.where(live, STORED | np.where(hit, REAL, 0) | np.where(pspec, SPECULAR, 0), 0)
        samples[s] = np.where(hit[:, None], smp, F(0))
        hits[s] = np.where(hit[:, None], ht, F(0))
        hits[s].view(np.int32)[:, 3] = np.where(hit, ht.view(np.int32)[:, 3], -1)
        live = hit
    return vertices, info, samples, hits


def kinds(info):
    """per step and item: (real, ghost, none) masks from the status words"""
    st = np.ascontiguousarray(info).view(np.uint32)[..., 3]
    return (st & REAL) != 0, ((st & STORED) != 0) & ((st & REAL) == 0), st == 0
