"""GPU tests of the frame's image-space tail on the edge-case images of tests/edge_images.py: bdpt_resolve /
bdpt_resolve_tile against the oracle and the exact rational reading, bdpt_accumulate / bdpt_accumulate_tile against the
oracle and the float32 restatement, bdpt_adaptive_update / bdpt_adaptive_reset against np_update — on every state family,
block size and small frame shape, on 32-frame sequences, and on a frame wide enough that the capped grids loop.  Every
comparison is bit for bit (a NaN equals any NaN: edge_images.same_bits)."""
import ctypes as C

import numpy as np
import pytest

import edge_images as ei
from edge_images import F, SENTINEL

pytestmark = pytest.mark.gpu

RW, RH = 37, 23        # the resolve / accumulate frame
BAND = (5, 18)         # rows 5 .. 17
STRIPES = (4, 3, 2)    # stripes of 4 rows dealt to 3 owners; owner 2 holds rows 8 .. 11 and the short last stripe 20 .. 22
MAX_WAVES = 2048       # launchAdaptiveUpdate's grid cap; launchAdaptiveReset's is 2048 blocks of 256 threads


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.tensor(a, device="cuda")


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


# ---- contexts of the 37 x 23 frame ---------------------------------------------------------------------------------------
class Shape:
    """a context of one tile shape, the frame pixels of its tile in tile order, and where each pixel's splat words live"""

    def __init__(self, pkg, kind):
        self.kind, self.ctx = kind, pkg.Context(0)
        if kind == "whole":
            self.ctx.resize(RW, RH, 0, RH, 1)
            rows = list(range(RH))
        elif kind == "band":
            self.ctx.resize(RW, RH, BAND[0], BAND[1], 1)
            rows = list(range(*BAND))
        else:
            self.ctx.resize_stripes(RW, RH, STRIPES[0], STRIPES[1], STRIPES[2], 1)
            rows = [y for a, b in self.ctx.row_ranges() for y in range(a, b)]
            assert rows == [8, 9, 10, 11, 20, 21, 22]
        self.pix = np.array([y * RW + x for y in rows for x in range(RW)], np.int64)
        info = self.ctx.tile_info()
        assert info.numPixels == len(self.pix)
        self.splat_u64 = int(info.splatU64)
        self.chunk_rows = int(info.chunkRows)

    def owner_major(self, words_frame):
        """the frame's words in this context's splat layout (kernels.h splatIndex); frame order unless striped"""
        if self.kind != "stripes":
            return words_frame
        R, owners, _ = STRIPES
        buf = np.zeros((self.splat_u64 // 4, 4), np.uint64)
        y, x = np.divmod(np.arange(RW * RH), RW)
        s = y // R
        buf[((s % owners) * self.chunk_rows + (s // owners) * R + (y - s * R)) * RW + x] = words_frame
        return buf


@pytest.fixture(scope="module")
def shapes(pkg):
    import torch
    assert torch.cuda.is_available()
    made = {k: Shape(pkg, k) for k in ("whole", "band", "stripes")}
    yield made
    for s in made.values():
        s.ctx.close()


@pytest.fixture(scope="module")
def resolve_case(pkg, ob):
    """Every family's rows dealt to the pixels of the frame, and the oracle's answer for the whole frame (== the exact
    reading, asserted here once)."""
    words, out, label, exact = ei.all_word_rows()
    row = ei.deal(len(words), RW * RH)
    scene = pkg.Scene.cornell()
    orc = ob.OracleRender(pkg.abi, scene.desc, RW, RH)
    orc.splat[:] = words[row]
    orc.chan["out"][:] = out[row]
    orc.resolve()
    want = orc.chan["out"].copy()
    orc.close()
    scene.close()
    assert ei.same_bits(want, exact[row]) and not np.isnan(want).any()
    return dict(words=words[row], out=out[row], label=label[row], want=want)


RESOLVES = ("whole", "band row0 0", "band row0 5", "stripes", "stripes tile-local")


@pytest.mark.parametrize("how", RESOLVES)
def test_resolve_equals_oracle(pkg, shapes, resolve_case, how):
    import torch
    sh = shapes[how.split()[0]]
    rc = resolve_case
    tile = np.zeros(RW * RH, bool)
    tile[sh.pix] = True
    landed = tile & (rc["words"][:, 3] != 0)
    # pixels outside the tile, and pixels nothing landed on, start as the sentinel and must keep it
    start = np.where(landed[:, None], rc["out"], SENTINEL).astype(F)
    out = _dev(torch, start)
    if how == "stripes tile-local":
        splat = _dev(torch, rc["words"][sh.pix])
        sh.ctx.resolve_tile(_ptr(splat), _ptr(out))
    elif how == "band row0 5":
        splat = _dev(torch, rc["words"][BAND[0] * RW:])
        sh.ctx.resolve(_ptr(splat), BAND[0], _ptr(out))
    else:
        splat = _dev(torch, sh.owner_major(rc["words"]))
        sh.ctx.resolve(_ptr(splat), 0, _ptr(out))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    differ = landed & (ei.bits(got) != ei.bits(rc["want"])).any(axis=1)
    written = ~landed & (got != SENTINEL).any(axis=1)
    names = lambda sel: sorted({ei.WORD_FAMILIES[i] for i in rc["label"][sel]})  # noqa: E731
    assert not differ.any() and not written.any(), (
        f"{how}: {int(differ.sum())} pixels differ from the oracle (families {names(differ)}); {int(written.sum())} pixels without a splat "
        f"or outside the tile were written ({int((written & tile).sum())} of them inside it, families {names(written & tile)})")
    # the case is not trivial: every family lands in the tile, untouched pixels exist inside and (but for `whole`) outside it
    assert set(rc["label"][tile].tolist()) == set(range(len(ei.WORD_FAMILIES))), how
    assert (tile & ~landed).sum() >= 3 and (how == "whole" or (~tile).sum() > RW)
    assert (got[landed] == 0).any() and (got[landed] == 1).any() and ((got[landed] > 0) & (got[landed] < 1)).any()


# ---- accumulate -------------------------------------------------------------------------------------------------------
def _oracle_accumulate(pkg, ob, last, cur, n, nmax):
    lib = ob.load_oracle(pkg.abi)
    a, b = np.ascontiguousarray(last, F).copy(), np.ascontiguousarray(cur, F).copy()
    lib.oracle_accumulate(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), n, nmax, len(a))
    return a


@pytest.mark.parametrize("family", ei.ACC_FAMILIES)
def test_accumulate_equals_oracle(pkg, ob, gpu_ctx, family):
    import torch
    classes = set()
    for last, cur, n, nmax in ei.acc_family(family):
        want = _oracle_accumulate(pkg, ob, last, cur, n, nmax)
        assert ei.same_bits(want, ei.accumulate_f32(last, cur, n, nmax))
        a, b = _dev(torch, last), _dev(torch, cur)
        gpu_ctx.accumulate(_ptr(a), _ptr(b), n, nmax, len(last))
        torch.cuda.synchronize()
        assert ei.same_bits(a.cpu().numpy(), want), (family, n, nmax, "last")
        assert ei.same_bits(b.cpu().numpy(), want), (family, n, nmax, "cur")
        classes |= set(np.unique(ei.value_class(want)).tolist())
    need = {"huge": {1, 2, 6}, "specials": {0, 1, 2, 3, 4, 6}, "cancel": {0, 1, 5}}.get(family, {1})
    assert need <= classes, (family, classes)


@pytest.mark.parametrize("kind", ["band", "stripes"])
def test_accumulate_tile_equals_oracle(pkg, ob, shapes, kind):
    import torch
    sh = shapes[kind]
    tile = np.zeros(RW * RH, bool)
    tile[sh.pix] = True
    cases = 0
    for family in ei.ACC_FAMILIES:
        for last, cur, n, nmax in ei.acc_family(family):
            row = ei.deal(len(last), RW * RH, seed=cases)
            want = _oracle_accumulate(pkg, ob, last[row], cur[row], n, nmax)
            a = _dev(torch, np.where(tile[:, None], last[row], SENTINEL).astype(F))
            b = _dev(torch, np.where(tile[:, None], cur[row], SENTINEL).astype(F))
            sh.ctx.accumulate_tile(_ptr(a), _ptr(b), n, nmax)
            torch.cuda.synchronize()
            for name, t in (("last", a), ("cur", b)):
                got = t.cpu().numpy()
                assert ei.same_bits(got[tile], want[tile]), (kind, family, n, nmax, name)
                assert (got[~tile] == SENTINEL).all(), (kind, family, n, nmax, name)
            cases += 1
    assert cases > 30 and 0 < tile.sum() < RW * RH


# ---- the adaptive update ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def adaptive_ctx(pkg):
    """a context with the Cornell scene; each test resizes it to its frame (whole frame, depth 1)"""
    scene = pkg.Scene.cornell()
    ctx = pkg.Context(0)
    ctx.set_scene(scene.desc)
    ctx.set_camera(scene.camera(1.0))
    yield ctx
    ctx.close()
    scene.close()


class DeviceState:
    def __init__(self, pkg, torch, st):
        self.t = {k: _dev(torch, st[k]) for k in ("mean", "m2", "count", "mask")}
        self.t["active"] = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        self.c = pkg.abi.AdaptiveState(*[self.t[k].data_ptr() for k in ("mean", "m2", "count", "mask", "active")])

    def differences(self, exp, frame, label):
        """what differs from the expected (mean, m2, count, mask, active, frame), as a list of messages"""
        mean, m2, count, mask, active, shown = exp
        got_active = int(self.t["active"].item())
        same = {"mean": ei.same_bits(self.t["mean"].cpu().numpy(), mean), "m2": ei.same_bits(self.t["m2"].cpu().numpy(), m2),
                "count": np.array_equal(_host(self.t["count"], np.uint32), count),
                "mask": np.array_equal(self.t["mask"].cpu().numpy(), mask),
                f"active {got_active}, expected {active}": got_active == active,
                "frame": frame is None or ei.same_bits(frame.cpu().numpy(), shown)}
        return [f"{label}: {k}" for k, ok in same.items() if not ok]

    def check(self, exp, frame, label):
        wrong = self.differences(exp, frame, label)
        assert not wrong, wrong


def _aparams(pkg, P, B):
    return pkg.abi.AdaptiveParams(float(P["threshold"]), float(P["epsilon"]), int(P["mn"]), int(P["mx"]), int(B))


def _np(st, P, B):
    return ei.np_update(st["mean"], st["m2"], st["count"], st["mask"], st["frame"], P["threshold"], P["epsilon"], P["mn"], P["mx"], B)


@pytest.mark.parametrize("shape", ei.SHAPES, ids=[f"{w}x{h}" for w, h in ei.SHAPES])
def test_update_equals_numpy_on_every_family(pkg, adaptive_ctx, shape):
    import torch
    W, H = shape
    adaptive_ctx.resize(W, H, 0, H, 1)
    seen_active, classes, wrong = set(), set(), []  # (wrong: every difference of every family, asserted empty below)
    for family in ei.STATE_FAMILIES:
        for label, st, P in ei.adaptive_states(family, W, H):
            for B in ei.BLOCKS:
                exp = _np(st, P, B)
                d = DeviceState(pkg, torch, st)
                fr = _dev(torch, st["frame"])
                adaptive_ctx.adaptive_update(_aparams(pkg, P, B), d.c, _ptr(fr))
                torch.cuda.synchronize()
                wrong += d.differences(exp, fr, f"{family} {label} B {B}".replace("  ", " "))
                if 0 < exp[4] < W * H:
                    seen_active.add((family, B))
            classes |= set(np.unique(ei.value_class(exp[0])).tolist()) | set(np.unique(ei.value_class(exp[1])).tolist())
    assert not wrong, (f"{W}x{H}: {len(wrong)} differences from np_update, in {sorted({w.split(' B ')[0] for w in wrong})}; "
                       f"the first: {wrong[:6]}")
    # not trivial: the ordinary state leaves some pixels active and some not at every block size the frame holds more than
    # one block of (one pixel, or one block, can only be all or nothing); NaN, infinities, zeros and negative values went through
    if W * H > 1:
        assert ("ordinary", 1) in seen_active and {0, 1, 2, 3, 5} <= classes, (seen_active, classes)
    if W > 8 and H > 8:
        assert all(("ordinary", B) in seen_active for B in (1, 2, 4, 8)), seen_active
    if W > 16 and H > 16:
        assert ("ordinary", 16) in seen_active


@pytest.mark.parametrize("family", ei.SEQ_FAMILIES)
def test_sequences_equal_numpy(pkg, adaptive_ctx, family):
    """K frames from bdpt_adaptive_reset on; an inactive pixel of the frame buffer keeps the mean the last update wrote
    there, as the masked frame leaves it."""
    import torch
    W, H = 67, 45
    adaptive_ctx.resize(W, H, 0, H, 1)
    frames = ei.sequence_frames(family, W, H)
    steps = ei.run_sequence(frames)
    junk = dict(mean=np.full((H, W, 4), 3, F), m2=np.full((H, W), 3, F), count=np.full((H, W), 3, np.uint32), mask=np.zeros((H, W), np.uint8))
    d = DeviceState(pkg, torch, junk)
    adaptive_ctx.adaptive_reset(d.c)
    torch.cuda.synchronize()
    z = ei.reset_state(H, W)
    d.check((z["mean"], z["m2"], z["count"], z["mask"], W * H, None), None, "reset")
    fr = torch.zeros(H, W, 4, dtype=torch.float32, device="cuda")
    P, params = ei.SEQ_PARAMS, _aparams(pkg, ei.SEQ_PARAMS, ei.SEQ_BLOCK)
    for k, s in enumerate(steps):
        on = _dev(torch, s["mask_in"] != 0)
        fr[on] = _dev(torch, frames[k])[on]
        adaptive_ctx.adaptive_update(params, d.c, _ptr(fr))
        torch.cuda.synchronize()
        d.check((s["mean"], s["m2"], s["count"], s["mask"], s["active"], s["mean"]), fr, f"{family} frame {k}")
    active = [s["active"] for s in steps]
    assert active[P["mn"] - 2] == W * H and active[-1] < W * H and all(b <= a for a, b in zip(active, active[1:]))


# ---- the capped grids ---------------------------------------------------------------------------------------------------
def _waves_with_nothing(mask, T):
    """(waves that find no active pixel in any of their tiles, waves that find some, fewest tiles of a wave): wave w of
    adaptive_update_kernel takes the tiles w, w + 2048, ... of T x T pixels, in row-major tile order"""
    H, W = mask.shape
    ty, tx = (H + T - 1) // T, (W + T - 1) // T
    pad = np.zeros((ty * T, tx * T), np.int64)
    pad[:H, :W] = mask
    per_tile = pad.reshape(ty, T, tx, T).sum(axis=(1, 3)).ravel()
    waves = min(len(per_tile), MAX_WAVES)
    per_wave = np.array([per_tile[w::waves].sum() for w in range(waves)])
    return int((per_wave == 0).sum()), int((per_wave > 0).sum()), len(per_tile) // waves


def test_wide_frame_loops_in_update_and_reset(pkg, adaptive_ctx):
    """32785 x 17: 557 345 pixels (the reset's 2048 x 256 threads loop), 4099 x 3 tiles of 8 and 2050 x 2 tiles of 16 (every
    wave of either update instance takes more than one tile and carries its count across them), partial tiles on the
    right and bottom edges.  Three updates in a row: `active` is right each time, so the scratch words were re-zeroed."""
    import torch
    W, H = ei.WIDE
    assert W * H > MAX_WAVES * 256 and ((W + 15) // 16) * ((H + 15) // 16) > MAX_WAVES and W % 16 and H % 16 and W % 8 and H % 8
    adaptive_ctx.resize(W, H, 0, H, 1)  # (accepted as it is: fewer than 2^24 pixels)
    (_, st, P), = ei.adaptive_states("ordinary", W, H)
    # converged columns such that whole waves of either instance meet converged tiles only: tiles of 8 with tx < 1000 or
    # 2050 <= tx < 3050 (wave w takes tx = w, w - 3, w - 6 and the same + 2048, + 2045, + 2042), tiles of 16 with tx < 500
    st["count"][:, :8000] = P["mx"]
    st["count"][:, 16400:24400] = P["mx"]
    rng = np.random.default_rng(9)
    for B in (8, 16):
        junk = dict(mean=np.full((H, W, 4), 3, F), m2=np.full((H, W), 3, F), count=np.full((H, W), 3, np.uint32),
                    mask=np.zeros((H, W), np.uint8))
        d = DeviceState(pkg, torch, junk)
        adaptive_ctx.adaptive_reset(d.c)
        torch.cuda.synchronize()
        z = ei.reset_state(H, W)
        d.check((z["mean"], z["m2"], z["count"], z["mask"], W * H, None), None, f"B {B}: reset")
        d = DeviceState(pkg, torch, st)
        cur = dict(st)
        for it in range(3):
            noise = (rng.random((H, W, 4), dtype=F) - F(0.5)) * F(0.3)
            cur["frame"] = (cur["mean"] + noise).astype(F)
            exp = _np(cur, P, B)
            fr = _dev(torch, cur["frame"])
            adaptive_ctx.adaptive_update(_aparams(pkg, P, B), d.c, _ptr(fr))
            torch.cuda.synchronize()
            d.check(exp, fr, f"B {B} update {it}")
            assert 0 < exp[4] < W * H
            nothing, some, tiles_per_wave = _waves_with_nothing(exp[3], 16 if B == 16 else 8)
            assert nothing >= 100 and some >= 100 and tiles_per_wave >= 2, (B, it, nothing, some, tiles_per_wave)
            cur = dict(mean=exp[0], m2=exp[1], count=exp[2], mask=exp[3])
