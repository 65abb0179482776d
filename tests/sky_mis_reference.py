"""MIS sky lighting outside the kernels (include/bdpt.h "Environment lighting", bdpt_bsdf_pdf_query and bdpt_sky_mis_query):
the density query's formulas in torch fp32 on the CPU (every operation its own correctly rounded step, as the device code
is compiled) and in numpy float64, and the composed loop the fused pass equals bit for bit — the queries on the device, the
elementwise arithmetic between them in numpy fp32.  Shared by tests/test_gpu_sky_mis.py."""
import numpy as np

import env_numpy as en
from walk_loop import gpu, host

F, U, D = np.float32, np.uint32, np.float64
KPI, KINVPI = F(3.14159265358979323846), F(0.318309886183790671538)
LUM = (F(0.2126), F(0.7152), F(0.0722))


# ---- torch fp32 (CPU) ------------------------------------------------------------------------------------------------
def fcos_pdf_torch(surf, dirs, mat):
    """bsdfFcosPdf of csrc/device_bsdf_pdf.hpp for (n, 24) records toward dirs[:, 0:3] -> (n, 4) float32 (fcos, pdf); a
    record with prim < 0 gives zeros"""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, F))
    surf = np.ascontiguousarray(surf, F)
    N, lr, V, dif, spec, L = t(surf[:, 4:7]), t(surf[:, 7]), t(surf[:, 8:11]), t(surf[:, 12:15]), t(surf[:, 16:19]), t(dirs[:, 0:3])
    n = len(surf)
    c = lambda v, like: torch.full_like(like, float(F(v)))  # a constant as a tensor: a true division, not a reciprocal
    zero, one = torch.zeros(n), torch.ones(n)
    dot = lambda a, b: (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]

    def sat(x):
        y = torch.where(x > 0, x, zero)
        return torch.where(y < 1, y, one)

    def maxf(a, b):  # HLSL max: the non-NaN operand wins
        return torch.where(b > a, b, torch.where(a == a, a, b))

    ndl = dot(N, L)
    NdotL = sat(ndl)
    if mat == 1:
        fcos = (NdotL[:, None] * dif) / c(KPI, dif)
        pdf = NdotL * c(KINVPI, NdotL)
    else:
        rough = lr * lr
        s = V + L
        # (torch's fp32 square root on the CPU is a vector routine that is not correctly rounded; the float64 one rounded
        # to fp32 is: 53 bits are more than twice 24 plus 2, so the second rounding cannot change the result)
        H = s * (one / torch.sqrt(dot(s, s).double()).float())[:, None]
        NdotH, LdotH, NdotV = sat(dot(N, H)), sat(dot(L, H)), sat(dot(N, V))
        a2 = rough * rough
        d = (NdotH * a2 - NdotH) * NdotH + one
        Dt = a2 / maxf(c(0.001, d), (d * d) * c(KPI, d))
        k = (rough * rough) / c(2, rough)
        g_v = NdotV / (NdotV * (one - k) + k)
        g_l = NdotL / (NdotL * (one - k) + k)
        G = g_v * g_l
        x = one - LdotH
        x2 = x * x
        p5 = (x2 * x2) * x
        Fr = spec + (torch.ones_like(spec) - spec) * p5[:, None]
        ggx = ((Dt * G)[:, None] * Fr) / (c(4, NdotV) * NdotV)[:, None]
        fcos = torch.ones_like(dif) * (ggx + (NdotL[:, None] * dif) / c(KPI, dif))

        def lum(rgb):
            return maxf(c(0.01, zero), (rgb[:, 0] * c(LUM[0], zero) + rgb[:, 1] * c(LUM[1], zero)) + rgb[:, 2] * c(LUM[2], zero))

        ld, ls = lum(dif), lum(spec)
        pd = ld / (ld + ls)
        pdfD = (NdotL * c(KINVPI, NdotL)) * pd
        pdfS = ((Dt * NdotH) / (c(4, LdotH) * LdotH)) * (one - pd)
        pdf = torch.where(ndl <= 0, zero, pdfD + pdfS)
    out = torch.cat([fcos, pdf[:, None]], dim=1).numpy().astype(F)
    out[surf.view(np.int32)[:, 23] < 0] = 0
    return out


# ---- numpy float64 (GGX, well-conditioned records) ---------------------------------------------------------------------
def ggx_fcos_pdf_f64(surf, dirs):
    """the GGX formulas read in float64, for records whose cosines are well away from 0 (no saturate or clamp is active)"""
    surf = np.asarray(surf, F).astype(D)
    N, lr, V, dif, spec, L = surf[:, 4:7], surf[:, 7], surf[:, 8:11], surf[:, 12:15], surf[:, 16:19], np.asarray(dirs, F)[:, 0:3].astype(D)
    dot = lambda a, b: (a * b).sum(axis=1)
    rough = lr * lr
    H = V + L
    H /= np.sqrt(dot(H, H))[:, None]
    NdotL, NdotV, NdotH, LdotH = dot(N, L), dot(N, V), dot(N, H), dot(L, H)
    a2 = rough * rough
    d = (NdotH * a2 - NdotH) * NdotH + 1.0
    Dt = a2 / (d * d * np.pi)
    k = rough * rough / 2.0
    G = (NdotV / (NdotV * (1 - k) + k)) * (NdotL / (NdotL * (1 - k) + k))
    Fr = spec + (1.0 - spec) * ((1.0 - LdotH) ** 5)[:, None]
    fcos = (Dt * G)[:, None] * Fr / (4.0 * NdotV)[:, None] + NdotL[:, None] * dif / np.pi
    w = np.array([0.2126, 0.7152, 0.0722], F).astype(D)  # the weights are fp32 constants
    ld, ls = np.maximum(D(F(0.01)), dif @ w), np.maximum(D(F(0.01)), spec @ w)
    pd = ld / (ld + ls)
    pdf = NdotL / np.pi * pd + Dt * NdotH / (4.0 * LdotH) * (1.0 - pd)
    return fcos, pdf, dict(NdotL=NdotL, NdotV=NdotV, LdotH=LdotH, a2=a2, d2pi=d * d * np.pi)


# ---- the composed loop ---------------------------------------------------------------------------------------------------
def mis_loop(ctx, surf, seeds, mat, techniques, clamps, snapshots, min_t, alive=None):
    """bdpt_sky_mis_query composed from the queries: per sample env_sample -> bsdf_pdf -> glue -> trace_rays("any") -> add,
    then sample_bsdf -> env_eval -> bsdf_pdf -> glue -> trace_rays("any") -> add.  numpy in; -> ({(clamp, samples): (color
    (n, 4), counts, seeds_out)} for every clamp of `clamps` and sample count of `snapshots`, traced (n,): the rays per item
    after the last sample).  The clamp only bounds a term, so one pass of the queries serves every clamp."""
    import torch
    surf = np.ascontiguousarray(surf, F)
    n = len(surf)
    surf_t = gpu(surf)
    live = surf.view(np.int32)[:, 23] >= 0
    if alive is not None:
        live = live & (np.asarray(alive) != 0)
    s = np.ascontiguousarray(seeds, U).copy()
    total = {c: np.zeros((n, 3), F) for c in clamps}
    cnt, traced = np.zeros(n, U), np.zeros(n, U)
    vis_t = torch.empty(n, dtype=torch.uint8, device="cuda")
    nxt_t = torch.empty(n, dtype=torch.int32, device="cuda")
    out = {}

    def add_terms(raw, pdf, rays):
        """raw: the unclamped quotient; pdf: the sampling technique's own density (0: the term is +0)"""
        nonlocal cnt, traced
        ctx.trace_rays(gpu(rays), "any", out=vis_t)
        torch.cuda.synchronize()
        vis = host(vis_t) != 0
        worth = None
        for c in clamps:
            term = np.where((pdf != 0)[:, None], en.clamp_vec(raw, c), F(0)).astype(F)
            w = live & (term != 0).any(axis=1)
            assert worth is None or np.array_equal(w, worth)  # the clamp does not change which terms are worth a ray
            worth = w
            with np.errstate(over="ignore"):  # (a record with an infinite colour sums to infinity, as in the kernel)
                total[c] = (total[c] + np.where((w & vis)[:, None], term, F(0))).astype(F)
        cnt = cnt + (worth & vis).astype(U)
        traced = traced + worth.astype(U)

    for k in range(1, max(snapshots) + 1):
        if techniques & 1:
            smp = host(ctx.env_sample(surf_t, gpu(s.view(np.int32)), mat_index=1, min_t=min_t, seeds_out=nxt_t))
            torch.cuda.synchronize()
            nxt = host(nxt_t).view(U).copy()
            fp = host(ctx.bsdf_pdf(surf_t, gpu(np.ascontiguousarray(smp[:, 4:8])), mat))
            pdf = smp[:, 11]
            pB = fp[:, 3] if techniques & 2 else np.zeros(n, F)
            with np.errstate(all="ignore"):
                raw = ((fp[:, 0:3] * smp[:, 8:11]).astype(F) / (pdf + pB).astype(F)[:, None]).astype(F)
            add_terms(raw, pdf, np.ascontiguousarray(smp[:, 0:8]))
            s = np.where(live, nxt, s)
        if techniques & 2:
            b = host(ctx.sample_bsdf(surf_t, gpu(s.view(np.int32)), mat, False))
            dirs = np.ascontiguousarray(b[:, 0:4])
            ev = host(ctx.env_eval(gpu(dirs)))
            fp = host(ctx.bsdf_pdf(surf_t, gpu(dirs), mat))
            pL = ev[:, 3] if techniques & 1 else np.zeros(n, F)
            with np.errstate(all="ignore"):
                raw = ((fp[:, 0:3] * ev[:, 0:3]).astype(F) / (pL + fp[:, 3]).astype(F)[:, None]).astype(F)
            rays = np.zeros((n, 8), F)
            rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = surf[:, 0:3], F(min_t), b[:, 0:3], F(1e38)
            add_terms(raw, b[:, 3], rays)
            s = np.where(live, en.draws(s, 3)[1], s)
        if k in snapshots:
            for c in clamps:
                color = np.ones((n, 4), F)
                with np.errstate(all="ignore"):
                    color[:, 0:3] = np.where(live[:, None], (total[c] / F(k)).astype(F), surf[:, 12:15])
                out[(c, k)] = (color, cnt.copy(), s.copy())
    return out, traced


def mis_query(ctx, surf, seeds, samples, mat, techniques, clamp, min_t, alive=None, count=None, fill=-7):
    """one bdpt_sky_mis_query into tensors filled with `fill` -> (color, counts, seeds_out) as numpy"""
    import torch
    n = len(surf)
    col = torch.full((n, 4), float(fill), dtype=torch.float32, device="cuda")
    counts = torch.full((n,), int(fill), dtype=torch.int32, device="cuda")
    sout = torch.full((n,), int(fill), dtype=torch.int32, device="cuda")
    res = ctx.sky_lighting_mis(gpu(np.ascontiguousarray(surf, F)), gpu(np.ascontiguousarray(seeds, U).view(np.int32)), samples, mat_index=mat,
                               techniques=techniques, clamp=clamp, min_t=min_t, alive=None if alive is None else gpu(alive), out=col,
                               counts=counts, seeds_out=sout, count=count)
    assert res is col
    torch.cuda.synchronize()
    return host(col), host(counts).view(U), host(sout).view(U)
