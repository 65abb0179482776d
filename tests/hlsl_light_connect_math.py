"""A second, independent reading of the reference's light evaluation and of its two connection strategies, per record,
in float64 numpy with the true acos — the sibling of hlsl_reference_math.py, used only to cross-check the oracle's fp32
restatement on edge-case records (tests/test_shading_edge_records_cpu.py).  Written from the shader files, not from the
oracle:

  evalPointLight / evalDirectionalLight / getDistanceFalloff     Falcor ShadingUtils/Lights.slang:54-102
  getLightData                                                   BDPT/Data/MaterialUtils.hlsli:67-85
  ggxDirect / lambertianDirect (a visible light)                 MaterialUtils.hlsli:149-184, 288-307
  evalGWithoutV, getUnweightedContribution (both path colours 1) BDPT/Data/BDPTUtils.hlsli:172-224
  getLaunchIndexFromDirection                                    BDPTUtils.hlsli:129-138
  the light-tracing splat's facing test, G and connectToCamera   BDPT/Data/BDPTMain.rt.hlsl:171-208, MaterialUtils.hlsli:10-13

Every function also returns the margins it met: for each comparison, the distance of the compared quantity from its
boundary, in that quantity's units.  A NaN margin is no boundary: a comparison with a NaN goes the same way in every
precision.  The uint() of a negative or out-of-frame pixel is out of range in HLSL; as in the oracle such a target is
dropped.
"""
import math

import numpy as np

import hlsl_reference_math as hm

M_PI = hm.M_PI
LIGHT_DIRECTIONAL = 1


def _norm(v):
    with np.errstate(all="ignore"):
        return v / np.float64(np.linalg.norm(v))


def _acos(x):
    """HLSL acos: NaN outside [-1, 1]"""
    if x != x or abs(x) > 1.0:
        return float("nan")
    return math.acos(x)


def select_light(seed, count):
    """-> (state after the draw, light, margin): the distance of r * count from the integers above and below it"""
    seed, r = hm.next_rand(seed)
    x = r * count
    inner = [abs(x - k) for k in range(1, count)]  # (0 and count are no boundaries: the draw is in [0, 1) and the index is clamped)
    return seed, min(int(x), count - 1), min(inner) if inner else float("inf")


def light_data(lt, hit):
    """lt: dict with type, posW, dirW, intensity, openingAngle, cosOpeningAngle, penumbraAngle.
    -> (toLight, intensity, distToLight, margins)"""
    lpos, ldir, inten = (np.array(lt[k], np.float64) for k in ("posW", "dirW", "intensity"))
    m = dict(dist2=float("inf"), cone=float("inf"), fp32_range=float("inf"), acos_domain=float("inf"))
    with np.errstate(all="ignore"):
        if lt["type"] == LIGHT_DIRECTIONAL:
            L = -_norm(ldir)
            dist = np.float64(np.linalg.norm(hit - lpos))
            ls_pos = hit - ldir * dist
            diffuse = inten
        else:
            L = lpos - hit
            d2 = float(np.dot(L, L))
            m["dist2"] = abs(d2 - 1e-5)
            # (an underflowing d2 takes the d2 <= 1e-5 branch in both precisions and vanishes beside 0.01^2: only overflow counts)
            m["fp32_range"] = hm.fp32_range_margin(d2) if d2 > 1.0 else float("inf")
            L = _norm(L) if d2 > 1e-5 else np.zeros(3)
            falloff = np.float64(1.0) / np.float64(0.01 * 0.01 + d2)
            cos_t = -float(np.dot(L, ldir))
            m["cone"] = abs(cos_t - lt["cosOpeningAngle"])
            if cos_t < lt["cosOpeningAngle"]:
                falloff = 0.0
            elif lt["penumbraAngle"] > 0:
                # Past 1 the shader's acos is outside its domain (NaN here, as on conforming hardware; within a rounding of
                # 1 it is the fp32 rounding that decides).  The build defines acos of the clamped argument there
                # (include/bdpt.h, bdpt_light_query): such a row is outside what this reading can arbitrate.
                if cos_t > 1.0 - 1e-6:
                    m["acos_domain"] = 0.5e-6
                delta = lt["openingAngle"] - _acos(cos_t)
                falloff = falloff * hm.saturate(float((delta - lt["penumbraAngle"]) / np.float64(lt["penumbraAngle"])))
            ls_pos, diffuse = lpos, inten * falloff
        return _norm(L), diffuse, float(np.linalg.norm(ls_pos - hit)), m


def direct_visible(mat_index, count, L, inten, n, v, dif, spec, rough):
    """ggxDirect / lambertianDirect with shadowMult = count -> (value, margins)"""
    with np.errstate(all="ignore"):
        ndl = float(np.dot(n, L))
        ndotl = hm.saturate(ndl)
        m = dict(ndotl=hm.cos_margin(n, L), ndotv=float("inf"))
        if mat_index == 1:
            return float(count) * ndotl * inten * dif / M_PI, m
        h = _norm(v + L)
        ndoth, ldoth = hm.saturate(float(np.dot(n, h))), hm.saturate(float(np.dot(L, h)))
        ndv = float(np.dot(n, v))
        m["ndotv"] = hm.cos_margin(n, v)
        ndotv = hm.saturate(ndv)
        term = hm.ggx_d(ndoth, rough) * hm.ggx_g(ndotl, ndotv, rough) * hm.schlick(spec, ldoth) / np.float64(4 * ndotv)
        return float(count) * inten * (term + ndotl * dif / M_PI), m


def light_nee(lights, seed, mat_index, pos, n, v, dif, spec, rough):
    """one NEE sample of a visible light -> (light, L, distance, value, margins)"""
    _, index, sel = select_light(seed, len(lights))
    L, inten, dist, m = light_data(lights[index], pos)
    value, m2 = direct_visible(mat_index, len(lights), L, inten, n, v, dif, spec, rough)
    m.update(m2, select=sel)
    return index, L, dist, value, m


def g_without_v(pa, na, pb, nb):
    with np.errstate(all="ignore"):
        vec = pb - pa
        inv = np.float64(1.0) / np.float64(np.linalg.norm(vec))
        d = vec * inv
        return abs(float(np.dot(na, d))) * abs(float(np.dot(nb, d))) * inv * inv


def connect_vertices(mat_index, eye, light, wo_e, wo_l):
    """eye / light: dicts with pos, N, dif, spec, rough, is_spec; wo_e / wo_l: the directions to the predecessors.
    -> (value, short cut taken (0 none, 1 fsL, 2 fsE), margins): (fsL * G) * fsE"""
    with np.errstate(all="ignore"):
        g = g_without_v(eye["pos"], eye["N"], light["pos"], light["N"])
        cd = _norm(eye["pos"] - light["pos"])
        m = dict(ndotl_light=hm.cos_margin(light["N"], wo_l), ndotl_eye=hm.cos_margin(eye["N"], wo_e),
                 ndotv_light=hm.cos_margin(light["N"], cd), ndotv_eye=hm.cos_margin(eye["N"], cd))
        if mat_index == 1:
            m = {k: float("inf") for k in m}
        len2 = float(np.dot(eye["pos"] - light["pos"], eye["pos"] - light["pos"]))
        m["fp32_range"] = hm.fp32_range_margin(len2, 1.0 / len2 if len2 > 0 else 0.0, g)
        fs_l = hm.eval_brdf(mat_index, cd, wo_l, light["N"], light["dif"], light["spec"], light["rough"], light["is_spec"])
        if (fs_l == 0).all():
            return fs_l, 1, m
        fs_e = hm.eval_brdf(mat_index, -cd, wo_e, eye["N"], eye["dif"], eye["spec"], eye["rough"], eye["is_spec"])
        if (fs_e == 0).all():
            return fs_e, 2, m
        return fs_l * g * fs_e, 0, m


def launch_index(cam, dir_, width, height, jitter):
    """cam: (pos, U, V, W) float64.  -> ((x, y) or None, margins): the four frame-edge comparisons and the rintf tie.
    Their unit is the frame: the compared quantity is pixelCenter in [0, 1), which fp32 forms with an error of a few
    1e-7 before it is scaled by the frame's size, so a margin is a distance in pixels over the width (height)."""
    _, U, V, Wv = cam
    inf = float("inf")
    with np.errstate(all="ignore"):
        d1 = np.float64(np.dot(dir_, U)) / np.float64(np.dot(U, U))
        d2 = np.float64(np.dot(dir_, V)) / np.float64(np.dot(V, V))
        d3 = np.float64(np.dot(dir_, Wv)) / np.float64(np.dot(Wv, Wv))
        gx = (d1 / d3) * 0.5 * width + 0.5 * width - jitter[0]
        gy = (-d2 / d3) * 0.5 * height + 0.5 * height - jitter[1]
    m = dict(left=inf, right=inf, top=inf, bottom=inf, tie=inf)
    if not (np.isfinite(gx) and np.isfinite(gy)):
        return None, m
    gx, gy = float(gx), float(gy)
    # round() to nearest: fx >= 0 is gx >= -0.5, fx < W is gx < W - 0.5 (up to the tie rule, which the tie margin covers)
    m.update(left=abs(gx + 0.5) / width, right=abs(gx - (width - 0.5)) / width, top=abs(gy + 0.5) / height,
             bottom=abs(gy - (height - 0.5)) / height,
             tie=min(abs(gx - math.floor(gx) - 0.5) / width, abs(gy - math.floor(gy) - 0.5) / height))
    ix, iy = np.rint(gx), np.rint(gy)
    if ix < 0 or iy < 0 or ix >= width or iy >= height:
        return None, m
    return (int(ix), int(iy)), m


def connect_camera(mat_index, cam, width, height, jitter, lv):
    """lv: dict with pos, N, V, dif, spec, rough, is_spec.  -> (pixel x + y * width or None, f, G, direction, distance, margins)"""
    cpos, _, _, Wv = cam
    with np.errstate(all="ignore"):
        cam_n = _norm(Wv)
        to = cpos - lv["pos"]
        d = _norm(to)
        dist = float(np.linalg.norm(to))
        face = float(np.dot(cam_n, d))
        m = dict(facing=abs(face), ndotl=float("inf"), ndotv=float("inf"), fp32_range=hm.fp32_range_margin(float(np.dot(to, to))))
        if not face < 0:
            return None, np.zeros(3), 0.0, d, dist, m
        target, m2 = launch_index(cam, d, width, height, jitter)
        m.update(m2)
        if target is None:
            return None, np.zeros(3), 0.0, d, dist, m
        t1 = hm.saturate(abs(float(np.dot(d, cam_n))))
        t2 = hm.saturate(abs(float(np.dot(d, lv["N"]))))
        inv = np.float64(1.0) / np.float64(dist)
        g = float(t1 * t2 * inv * inv)
        if mat_index == 0:
            m.update(ndotl=hm.cos_margin(lv["N"], d), ndotv=hm.cos_margin(lv["N"], lv["V"]))
        f = hm.eval_brdf(mat_index, lv["V"], d, lv["N"], lv["dif"], lv["spec"], lv["rough"], lv["is_spec"])
        return target[0] + target[1] * width, f, g, d, dist, m
