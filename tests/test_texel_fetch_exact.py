"""The texel fetches of device_scene.hpp against the formula they replaced (no GPU).

sampleBilinearT wraps with wrapT (a mask for a power-of-two side, the remainder otherwise) and wrapNext, and reads a row's
two texels with one 8-byte load of (ix0, ix0 + 1) plus a separate load of texel 0 in the wrap column; the alpha tests read
one word of the alpha-quad plane.  Each must pick exactly the texels, and hence the values, of the old wrapi / four-load /
four-byte formula for every input class: power-of-two and other sides, 1 x N textures, UVs far outside [0, 1] and
negative ones, sRGB and linear decode.

The C++ of csrc/texture_planes.h (wrapT, wrapNext, texPow2Flags, alphaSamplesTexture, alphaQuadRows: what both the device
samplers and the host set-up use) runs here through tests/host_compile/texture_planes_test.cpp, compiled with g++; the
row-pair load of texelRow, device-only, is restated in numpy.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fyp-bidirectionalpathtracer_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("texture_planes") / "texture_planes_test")
    src = os.path.join(ROOT, "tests", "host_compile", "texture_planes_test.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + CSRC, "-o", exe, src],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


SIDES = [1, 2, 3, 5, 7, 64, 100, 128, 255, 256, 512, 1000, 1024]


def wrapi(i, n):  # C's i % n (truncating) then + n where negative
    m = np.fmod(i, n)
    return np.where(m < 0, m + n, m)


def old_indices(x0, n):
    ix0 = wrapi(x0, n)
    return ix0, wrapi(ix0 + 1, n)


def new_indices(x0, n):
    pow2 = (n & (n - 1)) == 0
    ix0 = (x0 & (n - 1)) if pow2 else wrapi(x0, n)  # two's complement int32 and
    ix1 = np.where(ix0 + 1 == n, 0, ix0 + 1)
    return ix0, ix1


def floor_int(x0):
    """The samplers' (int)floorf(x) as include/bdpt.h "Surface queries" defines it outside the int range: saturating, NaN -> 0
    (csrc/texture_planes.h texelFloorInt; a plain astype(int32) is as undefined there as the C cast)."""
    x0 = np.asarray(x0, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x0), 0.0, np.clip(x0, -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64).astype(np.int32)


def coords(rng, n):
    """Integer floors (int)floorf(u * n - 0.5f) for UVs inside, near and far outside [0, 1], negative ones included."""
    u = np.concatenate([rng.uniform(0, 1, 4000), rng.uniform(-3, 4, 4000), rng.uniform(-1e4, 1e4, 2000),
                        np.array([0.0, 1.0, -1.0, 0.5 / n, 1 - 0.5 / n, -0.5 / n, 2.0, -2.0])]).astype(np.float32)
    x = u * np.float32(n) - np.float32(0.5)
    x0 = floor_int(np.floor(x))
    edge = np.array([-(2 ** 31), 2 ** 31 - 1, -(2 ** 31) + 1, -n, -n - 1, n, n - 1, 0, -1], dtype=np.int64)
    return np.concatenate([x0, edge.astype(np.int32)]).astype(np.int32)


@pytest.mark.parametrize("n", SIDES)
def test_wrap_by_mask_equals_remainder(n):
    rng = np.random.default_rng(n)
    x0 = coords(rng, n)
    o0, o1 = old_indices(x0, n)
    n0, n1 = new_indices(x0, n)
    np.testing.assert_array_equal(o0, n0)
    np.testing.assert_array_equal(o1, n1)
    assert ((n0 >= 0) & (n0 < n)).all()


def srgb_lut():
    c = np.arange(256) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4).astype(np.float32)


def decode(bytes4, srgb):
    rgb = bytes4[..., :3]
    out = np.empty(bytes4.shape, np.float32)
    out[..., :3] = srgb_lut()[rgb] if srgb else rgb.astype(np.float32) / np.float32(255.0)
    out[..., 3] = bytes4[..., 3].astype(np.float32) / np.float32(255.0)
    return out


def sample(tex, srgb, u, v, new):
    """sampleBilinearT in fp32, old texel addressing or the new one (pair load + wrap-column fix-up)."""
    h, w, _ = tex.shape
    x = u * np.float32(w) - np.float32(0.5)
    y = v * np.float32(h) - np.float32(0.5)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    if not new:
        ix0, ix1 = old_indices(floor_int(x0), w)
        iy0, iy1 = old_indices(floor_int(y0), h)
        t = [decode(tex[iy, ix], srgb) for iy, ix in ((iy0, ix0), (iy0, ix1), (iy1, ix0), (iy1, ix1))]
    else:
        ix0, ix1 = new_indices(floor_int(x0), w)
        iy0, iy1 = new_indices(floor_int(y0), h)
        flat = np.concatenate([tex.reshape(-1, 4), np.zeros((1, 4), np.uint8)])  # the texture's spare texel
        t = []
        for iy in (iy0, iy1):
            a = flat[iy * w + ix0]       # low word of the 8-byte load
            b = flat[iy * w + ix0 + 1]   # high word
            b = np.where((ix1 != ix0 + 1)[:, None], flat[iy * w + ix1], b)
            t += [decode(a, srgb), decode(b, srgb)]
    fx, fy = fx[:, None], fy[:, None]
    top = t[0] + (t[1] - t[0]) * fx
    bot = t[2] + (t[3] - t[2]) * fx
    return top + (bot - top) * fy


@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (7, 1), (1, 64), (64, 1), (3, 5), (256, 256), (100, 37), (512, 128)])
@pytest.mark.parametrize("srgb", [0, 1])
def test_bilinear_pair_loads_equal_four_loads(w, h, srgb):
    rng = np.random.default_rng(w * 1000 + h + srgb)
    tex = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    n = 6000
    u = np.concatenate([rng.uniform(0, 1, n), rng.uniform(-5, 6, n), rng.uniform(-3e3, 3e3, n)]).astype(np.float32)
    v = np.concatenate([rng.uniform(0, 1, n), rng.uniform(-5, 6, n), rng.uniform(-3e3, 3e3, n)]).astype(np.float32)
    old = sample(tex, srgb, u, v, new=False)
    new = sample(tex, srgb, u, v, new=True)
    assert old.view(np.uint32).tolist() == new.view(np.uint32).tolist()


def alpha_quad_plane(tex):  # texture_planes.h alphaQuadRows, restated
    h, w, _ = tex.shape
    a = tex[..., 3].astype(np.uint32)
    a10 = np.roll(a, -1, axis=1)
    a01 = np.roll(a, -1, axis=0)
    a11 = np.roll(a01, -1, axis=1)
    return (a | (a10 << 8) | (a01 << 16) | (a11 << 24)).reshape(-1)


@pytest.mark.parametrize("w,h", [(1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (256, 256), (100, 37)])
def test_alpha_quad_plane_equals_four_byte_loads(w, h):
    rng = np.random.default_rng(w * 7 + h)
    tex = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    quad = alpha_quad_plane(tex)
    n = 5000
    u = np.concatenate([rng.uniform(0, 1, n), rng.uniform(-4, 5, n), rng.uniform(-2e3, 2e3, n)]).astype(np.float32)
    v = np.concatenate([rng.uniform(0, 1, n), rng.uniform(-4, 5, n), rng.uniform(-2e3, 2e3, n)]).astype(np.float32)
    x0 = floor_int(np.floor(u * np.float32(w) - np.float32(0.5)))
    y0 = floor_int(np.floor(v * np.float32(h) - np.float32(0.5)))
    ix0, ix1 = old_indices(x0, w)
    iy0, iy1 = old_indices(y0, h)
    old = [tex[iy, ix, 3] for iy, ix in ((iy0, ix0), (iy0, ix1), (iy1, ix0), (iy1, ix1))]
    nx0, _ = new_indices(x0, w)
    ny0, _ = new_indices(y0, h)
    q = quad[ny0 * w + nx0]
    new = [(q >> s) & 0xFF for s in (0, 8, 16, 24)]
    for o, nn in zip(old, new):
        np.testing.assert_array_equal(o.astype(np.uint32), nn)


# ---- the C++ of texture_planes.h ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIDES)
def test_cpp_wrap_equals_remainder(harness, tmp_path, n):
    x0 = coords(np.random.default_rng(n + 99), n)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    x0.astype(np.int32).tofile(fin)
    r = subprocess.run([harness, "wrap", str(n), str(fin), str(fout)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(fout, dtype=np.int32).reshape(-1, 2)
    o0, o1 = old_indices(x0, n)
    np.testing.assert_array_equal(got[:, 0], o0)
    np.testing.assert_array_equal(got[:, 1], o1)


FLOOR_EDGES = np.array([0.0, -0.0, 1.0, -1.0, 2147483520.0, 2147483648.0, 2147483904.0, -2147483520.0, -2147483648.0, -2147483904.0,
                        1e12, -1e12, 3e38, -3e38, np.inf, -np.inf, np.nan, 16777216.0, -16777217.0], np.float32)


def test_cpp_float_to_int_saturates(harness, tmp_path):
    """texelFloorInt (the host spelling of the samplers' conversion) and floor_int above: the cast inside the int range,
    INT_MAX / INT_MIN beyond it, 0 for NaN; and the wrapped index of each is inside the texture for every side."""
    x0 = np.concatenate([FLOOR_EDGES, np.floor(np.random.default_rng(5).uniform(-3e9, 3e9, 2000)).astype(np.float32)])
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    x0.tofile(fin)
    r = subprocess.run([harness, "floor", str(fin), str(fout)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(fout, dtype=np.int32)
    np.testing.assert_array_equal(got, floor_int(x0))
    expect = {2147483520.0: 2147483520, 2147483648.0: 2 ** 31 - 1, 2147483904.0: 2 ** 31 - 1, -2147483648.0: -2 ** 31, -2147483904.0: -2 ** 31,
              1e12: 2 ** 31 - 1, -3e38: -2 ** 31, np.inf: 2 ** 31 - 1, -np.inf: -2 ** 31}
    for v, e in expect.items():
        assert got[np.flatnonzero(x0 == np.float32(v))[0]] == e, v
    assert got[np.flatnonzero(np.isnan(x0))[0]] == 0
    inside = np.abs(x0.astype(np.float64)) < 2.0 ** 31
    np.testing.assert_array_equal(got[inside], x0[inside].astype(np.int64))
    for n in SIDES:
        o0, _ = old_indices(got, n)
        n0, _ = new_indices(got, n)
        np.testing.assert_array_equal(o0, n0)
        assert ((n0 >= 0) & (n0 < n)).all()


def test_cpp_pow2_flags(harness):
    r = subprocess.run([harness, "flags"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    rows = [tuple(int(v) for v in line.split()) for line in r.stdout.split("\n") if line.strip()]
    assert len(rows) == 10
    for w, h, f in rows:
        assert f == (1 if w & (w - 1) == 0 else 0) | (2 if h & (h - 1) == 0 else 0), (w, h, f)


def test_cpp_alpha_rule_matches_sample_texture(harness):
    """alphaSamplesTexture is the rule of sampleTexture: every 3-bit diffuse type but UNUSED (0) and CONST (1) samples a
    present texture.  alpha_recs_kernel writes mode 2 under it and bdpt_set_scene makes the alpha-quad planes under it, so
    a mode-2 record never lacks its plane, for types 3-7 as much as for TEXTURE (2)."""
    r = subprocess.run([harness, "rule"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    rows = [tuple(int(v) for v in line.split()) for line in r.stdout.split("\n") if line.strip()]
    assert len(rows) == 16
    for typ, tex, samples in rows:
        assert samples == int(typ not in (0, 1) and tex >= 0), (typ, tex, samples)


@pytest.mark.parametrize("w,h", [(1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (256, 256), (100, 37), (7, 64)])
def test_cpp_alpha_quad_plane_equals_four_byte_loads(harness, tmp_path, w, h):
    rng = np.random.default_rng(w * 13 + h)
    tex = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(np.array([w, h], dtype=np.uint32).tobytes() + tex.tobytes())
    r = subprocess.run([harness, "plane", str(fin), str(fout)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    quad = np.fromfile(fout, dtype=np.uint32)
    assert quad.shape == (w * h,)
    # every texel as ix0, iy0 of a footprint: its quad holds the four alpha bytes the old formula loaded, low byte first
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    ix0, ix1 = old_indices(xs.reshape(-1).astype(np.int32), w)
    iy0, iy1 = old_indices(ys.reshape(-1).astype(np.int32), h)
    old = [tex[iy, ix, 3].astype(np.uint32) for iy, ix in ((iy0, ix0), (iy0, ix1), (iy1, ix0), (iy1, ix1))]
    q = quad[iy0 * w + ix0]
    for k, o in enumerate(old):
        np.testing.assert_array_equal((q >> (8 * k)) & 0xFF, o)
