"""Environment lighting in numpy (include/bdpt.h "Environment lighting"): the sampling table restated in exact integer
arithmetic (the per-texel f in fp32 as the header writes it, q through float64, the prefix sums as integers), the test maps,
ctypes wrappers of the host twins bdpt_host_env_table / _sample / _eval, the RNG's draws, a float64 reading of the sampler's
formulas, and the fp32 value arithmetic of bdpt_env_query and bdpt_sky_query.  Shared by test_env_cpu.py, test_gpu_env.py and
test_gpu_sky.py."""
import ctypes as C

import numpy as np

F, U, D = np.float32, np.uint32, np.float64
FLT_MAX = F(3.4028234663852886e38)
TINY = F(1.401298464324817e-45)
PI32 = F(3.14159265358979323846)
LCG_INV = 4276115653  # 1664525^-1 mod 2^32
NO_TEXEL = 0xFFFFFFFF


# ---- the RNG ---------------------------------------------------------------------------------------------------------
def lcg(s):
    return ((s.astype(np.uint64) * np.uint64(1664525) + np.uint64(1013904223)) & np.uint64(0xFFFFFFFF)).astype(U)


def lcg_back(s):
    return (((s.astype(np.uint64) + np.uint64(2**32 - 1013904223)) & np.uint64(0xFFFFFFFF)) * np.uint64(LCG_INV) & np.uint64(0xFFFFFFFF)).astype(U)


def draws(seeds, n=4):
    """-> (the n draws of nextRand as 24-bit integers (len, n), the state after them)"""
    s, out = np.asarray(seeds, U), []
    for _ in range(n):
        s = lcg(s)
        out.append(s & U(0x00FFFFFF))
    return np.stack(out, axis=1), s


def seeds_for_first_draw(r24):
    """states whose first draw is r24 / 2^24 (the later draws follow from it: an LCG's low bits are a function of its low bits)"""
    return lcg_back(np.asarray(r24, U))


# ---- fp32 functions of csrc/env_light.h ------------------------------------------------------------------------------
def sincos2pi(u):
    u = np.asarray(u, F)
    t = u * F(4.0)
    q = np.floor(t + F(0.5)).astype(F)
    r = t - q
    a = r * F(1.57079632679489661923)
    a2 = a * a
    sp = F(-1.0) / F(5040.0) + a2 * (F(1.0) / F(362880.0))
    sp = F(1.0) / F(120.0) + a2 * sp
    sp = F(-1.0) / F(6.0) + a2 * sp
    sp = F(1.0) + a2 * sp
    sa = a * sp
    cp = F(1.0) / F(40320.0) + a2 * (F(-1.0) / F(3628800.0))
    cp = F(-1.0) / F(720.0) + a2 * cp
    cp = F(1.0) / F(24.0) + a2 * cp
    cp = F(-0.5) + a2 * cp
    ca = F(1.0) + a2 * cp
    qi = q.astype(np.int64) & 3
    s0 = np.where(qi & 1, ca, sa)
    c0 = np.where(qi & 1, sa, ca)
    return np.where(qi & 2, -s0, s0).astype(F), np.where((qi == 1) | (qi == 2), -c0, c0).astype(F)


def sin_row(H):
    y = np.arange(H, dtype=F)
    return sincos2pi(((y + F(0.5)) / F(H)) * F(0.5))[0]


def texel_f(env):
    """f(x, y) of an (H, W, 4) float32 map, fp32 as envTexelF writes it"""
    env = np.asarray(env, F)
    H = env.shape[0]
    with np.errstate(all="ignore"):
        c = np.where(env[..., :3] > 0, np.minimum(env[..., :3], FLT_MAX), F(0)).astype(F)
        lit = (c > 0).any(axis=-1)
        lum = (c[..., 0] * F(0.2126) + c[..., 1] * F(0.7152)) + c[..., 2] * F(0.0722)
        lum = np.where(lum > 0, lum, TINY).astype(F)
        sr = sin_row(H)[:, None]
        f = (lum * sr).astype(F)
        f = np.where(f > 0, f, np.where(sr > 0, TINY, F(0))).astype(F)
        f = np.minimum(f, FLT_MAX)
    return np.where(lit, f, F(0)).astype(F)


def table(env):
    """-> dict(q (H, W) uint32, cdf (H, W) uint32, row_cdf (H,) uint64, total int, m float32), in exact integer arithmetic"""
    f = texel_f(env)
    m = f.max()
    q = np.zeros(f.shape, np.uint64)
    lit = f > 0
    if lit.any():
        ratio = f[lit].astype(D) / D(m)
        q[lit] = 1 + np.floor(ratio * 65535.0).astype(np.uint64)
    cdf = np.cumsum(q, axis=1, dtype=np.uint64)
    assert cdf.max(initial=0) < 2**32
    row_cdf = np.cumsum(cdf[:, -1], dtype=np.uint64)
    return dict(q=q.astype(U), cdf=cdf.astype(U), row_cdf=row_cdf, total=int(row_cdf[-1]), m=F(m))


def search(tab, r1, r2):
    """the sampler's texel for 24-bit draws r1, r2 (integers): numpy's searchsorted on the integer tables -> (x, y), or None
    when total == 0.  t and t2 in float64 as the header writes them (exact: a 24-bit integer times an integer below 2^44)."""
    total = tab["total"]
    if total == 0:
        return None
    t = np.minimum(np.floor((np.asarray(r1, D) / 16777216.0) * D(total)).astype(np.uint64), np.uint64(total - 1))
    y = np.searchsorted(tab["row_cdf"], t, side="right")
    row_total = tab["cdf"][y, -1].astype(np.uint64)
    t2 = np.minimum(np.floor((np.asarray(r2, D) / 16777216.0) * row_total.astype(D)).astype(np.uint64), row_total - np.uint64(1))
    x = np.array([np.searchsorted(tab["cdf"][yy], tt, side="right") for yy, tt in zip(y, t2)], np.int64)
    return x, y.astype(np.int64)


# ---- the maps --------------------------------------------------------------------------------------------------------
def sun_map():
    """a 64 x 32 sky with one texel at 1e6 and two all-zero rows"""
    rng = np.random.default_rng(21)
    env = np.zeros((32, 64, 4), F)
    env[..., :3] = rng.uniform(0.2, 1.0, (32, 64, 3)).astype(F) * np.array([0.5, 0.7, 1.0], F)
    env[..., 3] = 1
    env[5] = 0
    env[20] = 0
    env[9, 41, :3] = 1e6
    return env


SUN_TEXEL = (41, 9)


def random_map(W, H, seed):
    rng = np.random.default_rng(seed)
    env = np.ones((H, W, 4), F)
    env[..., :3] = rng.uniform(0.05, 2.0, (H, W, 3)).astype(F)
    return env


def edge_map():
    """NaN, +-inf, negative and subnormal texels beside ordinary ones"""
    nan, inf = F("nan"), F("inf")
    texels = [(nan, nan, nan), (nan, 1, 0), (inf, 0, 0), (-inf, 2, 0), (-1, -1, -1), (-1, 0.5, -3), (1e-45, 0, 0), (0, 0, 1e-45),
              (1e-40, 1e-41, 1e-45), (0, 0, 0), (-0.0, -0.0, -0.0), (3e38, 3e38, 3e38), (inf, inf, inf), (1, 1, 1), (1e-20, 0, 0),
              (0, nan, 5)]
    env = np.zeros((4, 4, 4), F)
    env[..., :3] = np.array(texels, F).reshape(4, 4, 3)
    return env


def subnormal_map():
    """only subnormal channels: the maximum itself is subnormal"""
    env = np.zeros((3, 5, 4), F)
    env[..., :3] = np.array([1e-45, 3e-45, 1e-42], F)
    env[1, 2, :3] = 0
    return env


def maps(row_chunk, marginal_chunk):
    """the maps of the CPU list, by name: {name: (H, W, 4) float32}"""
    out = {"1x1": random_map(1, 1, 1), "2x1": random_map(2, 1, 2), "1x2": random_map(1, 2, 3), "7x5": random_map(7, 5, 4),
           "sun": sun_map(), "edge": edge_map(), "subnormal": subnormal_map(), "zero": np.zeros((3, 4, 4), F),
           "wide": random_map(row_chunk + 1, 2, 5), "tall": random_map(2, marginal_chunk + 1, 6)}
    wide2 = random_map(2 * row_chunk + 3, 2, 7)  # two carries, and a run of dark texels across the first
    wide2[0, row_chunk - 2:row_chunk + 2, :3] = 0
    out["wide2"] = wide2
    return out


# ---- the host twins --------------------------------------------------------------------------------------------------
def host_table(lib, env):
    env = np.ascontiguousarray(env, F)
    H, W = env.shape[:2]
    q, cdf, row = np.zeros((H, W), U), np.zeros((H, W), U), np.zeros(H, np.uint64)
    m = C.c_float()
    rc = lib.bdpt_host_env_table(env.ctypes.data, W, H, q.ctypes.data, cdf.ctypes.data, row.ctypes.data, C.byref(m))
    assert rc == 0, rc
    return dict(q=q, cdf=cdf, row_cdf=row, total=int(row[-1]), m=F(m.value))


SAMPLE_DT = np.dtype([("dir", F, 3), ("pdf", F), ("radiance", F, 3), ("texel", U)])
EVAL_DT = np.dtype([("radiance", F, 3), ("pdf", F), ("texel", U), ("reserved", U, 3)])


def host_sample(lib, env, tab, seeds):
    env, seeds = np.ascontiguousarray(env, F), np.ascontiguousarray(seeds, U)
    H, W = env.shape[:2]
    cdf, row = np.ascontiguousarray(tab["cdf"], U), np.ascontiguousarray(tab["row_cdf"], np.uint64)
    out, sout = np.zeros(len(seeds), SAMPLE_DT), np.zeros(len(seeds), U)
    rc = lib.bdpt_host_env_sample(env.ctypes.data, W, H, cdf.ctypes.data, row.ctypes.data, seeds.ctypes.data, len(seeds), out.ctypes.data,
                                  sout.ctypes.data)
    assert rc == 0, rc
    return out, sout


def host_eval(lib, env, tab, dirs):
    env = np.ascontiguousarray(env, F)
    H, W = env.shape[:2]
    d4 = np.zeros((len(dirs), 4), F)
    d4[:, :3] = np.asarray(dirs, F)[:, :3]
    cdf, row = np.ascontiguousarray(tab["cdf"], U), np.ascontiguousarray(tab["row_cdf"], np.uint64)
    out = np.zeros(len(d4), EVAL_DT)
    rc = lib.bdpt_host_env_eval(env.ctypes.data, W, H, cdf.ctypes.data, row.ctypes.data, d4.ctypes.data, len(d4), out.ctypes.data)
    assert rc == 0, rc
    return out


# ---- a float64 reading of the sampler ------------------------------------------------------------------------------------
def f64_sample(tab, W, H, x, y, r3, r4):
    """dir, pdf and sin(theta) of texel (x, y) with the 24-bit draws r3, r4, in float64 with the true sin / cos; the draws
    and u, v themselves are exact in float64"""
    u = (x.astype(D) + r3.astype(D) / 16777216.0) / W
    v = (y.astype(D) + r4.astype(D) / 16777216.0) / H
    st, ct = np.sin(np.pi * v), np.cos(np.pi * v)
    s, c = np.sin(2 * np.pi * u), np.cos(2 * np.pi * u)
    q = tab["q"][y, x].astype(D)
    with np.errstate(all="ignore"):
        pdf = np.where(st > 0, (q / D(tab["total"])) * (W * H) / (2 * np.pi * np.pi * st), 0.0)
    return np.stack([-st * s, ct, st * c], axis=1), pdf, st, u * W, v * H


def border_distance(uw, vh):
    """how far (u W, v H) lies from a texel border, in texels"""
    return np.minimum(np.abs(uw - np.round(uw)), np.abs(vh - np.round(vh)))


# ---- the fp32 value arithmetic of bdpt_env_query / bdpt_sky_query ------------------------------------------------------
def _sat(x):
    with np.errstate(all="ignore"):
        y = np.where(x > 0, x, F(0)).astype(F)
        return np.where(y < 1, y, F(1)).astype(F)


def _dot(a, b):
    with np.errstate(all="ignore"):
        return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]).astype(F)


def clamp_vec(v, hi):
    with np.errstate(all="ignore"):
        y = np.where(v > 0, v, F(0)).astype(F)
        return np.where(y < F(hi), y, F(hi)).astype(F)


def lambert_value(N, dirs, radiance, diffuse, pdf):
    """(((NdotL * radiance) * diffuse) / kPi) / pdf in fp32, +0 where pdf == 0"""
    with np.errstate(all="ignore"):
        ndotl = _sat(_dot(N, dirs))[:, None]
        v = ((((ndotl * radiance).astype(F) * diffuse).astype(F) / PI32).astype(F) / pdf[:, None]).astype(F)
    return np.where((pdf != 0)[:, None], v, F(0)).astype(F)


def _normalize(a):
    with np.errstate(all="ignore"):
        inv = (F(1.0) / np.sqrt(_dot(a, a)).astype(F)).astype(F)
        return (a * inv[:, None]).astype(F)


def _maxf(a, b):  # HLSL max: the non-NaN operand wins
    with np.errstate(all="ignore"):
        return np.where(b > a, b, np.where(a == a, a, b)).astype(F)


def ggx_value(N, V, dirs, radiance, diffuse, spec, lin_rough, pdf):
    """directIfVisible<GGX>(1, L = dirs, intensity = radiance, ...) / pdf in fp32 as device_math.hpp writes it, +0 where pdf == 0"""
    with np.errstate(all="ignore"):
        rough = (lin_rough * lin_rough).astype(F)
        ndotl = _sat(_dot(N, dirs))
        Hh = _normalize((V + dirs).astype(F))
        ndoth, ldoth, ndotv = _sat(_dot(N, Hh)), _sat(_dot(dirs, Hh)), _sat(_dot(N, V))
        a2 = (rough * rough).astype(F)
        d = (((ndoth * a2).astype(F) - ndoth).astype(F) * ndoth + F(1)).astype(F)
        Dt = (a2 / _maxf(np.full_like(d, F(0.001)), ((d * d).astype(F) * PI32).astype(F))).astype(F)
        k = ((rough * rough).astype(F) / F(2)).astype(F)
        g_v = (ndotv / ((ndotv * (F(1) - k)).astype(F) + k).astype(F)).astype(F)
        g_l = (ndotl / ((ndotl * (F(1) - k)).astype(F) + k).astype(F)).astype(F)
        G = (g_v * g_l).astype(F)
        x = (F(1.0) - ldoth).astype(F)
        x2 = (x * x).astype(F)
        p5 = ((x2 * x2).astype(F) * x).astype(F)
        Fr = (spec + ((F(1.0) - spec).astype(F) * p5[:, None]).astype(F)).astype(F)
        ggx = (((Dt * G).astype(F)[:, None] * Fr).astype(F) / (F(4) * ndotv).astype(F)[:, None]).astype(F)
        lam = ((ndotl[:, None] * diffuse).astype(F) / PI32).astype(F)
        val = ((F(1.0) * radiance).astype(F) * (ggx + lam).astype(F)).astype(F)
        v = (val / pdf[:, None]).astype(F)
    return np.where((pdf != 0)[:, None], v, F(0)).astype(F)
