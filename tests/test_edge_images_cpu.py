"""CPU checks of the frame's image-space tail on edge-case images (tests/edge_images.py): the oracle's resolve against an
exact rational reading and a float64 one, its running mean against the float32 restatement and float64, and the float32
restatement of the adaptive update against a float64 mean and two-pass variance of the same frames.

    python tests/test_edge_images_cpu.py      prints MEASURED, MARGIN and LEFT_OUT for tests/edge_images.py
"""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import edge_images as ei
from edge_images import F

SEQ_SHAPE = (67, 45)  # W x H: the frame the GPU test runs the sequences on
WELL_LEFT_OUT = 0.01  # a well-conditioned family may leave out at most 1 % of its pixel-updates
ILL_LEFT_OUT = 0.5    # an ill-conditioned one at most half


def test_numpy_keeps_subnormals():
    assert ei.keeps_subnormals()


# ---- round_f32 --------------------------------------------------------------------------------------------------------
def _f32_bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def test_round_f32_against_numpy():
    """A double is exact as a Fraction and numpy rounds it to float32 once: the helper must give the same bits on random
    doubles of every magnitude and around every boundary (ties, subnormals, underflow to zero, overflow to inf)."""
    rng = np.random.default_rng(1)
    x = rng.uniform(1.0, 2.0, 4000) * 2.0 ** rng.integers(-160, 135, 4000) * rng.choice([-1.0, 1.0], 4000)
    edge = []
    for m in (2 ** 24 + 1, 2 ** 24 + 3, 2 ** 25 - 1, 2 ** 23, 2 ** 24 - 1, 1, 3):
        for e in (-175, -174, -173, -172, -151, -150, -149, -126, -30, 0, 39, 100, 103, 104):
            for d in (-2.0 ** -28, 0.0, 2.0 ** -28):  # (m + d is exact in a double: m < 2^25)
                edge.append((m + d) * 2.0 ** e)
    fmax = float(np.finfo(np.float32).max)
    edge += [fmax, fmax + 2.0 ** 102, np.nextafter(fmax + 2.0 ** 103, 0), fmax + 2.0 ** 103, 2.0 ** 128, 1e300, 2.0 ** -149, 2.0 ** -150,
             np.nextafter(2.0 ** -150, 1), 2.0 ** -126, np.nextafter(2.0 ** -126, 0), 5e-324]
    x = np.concatenate([x, np.array(edge), -np.array(edge)])
    with np.errstate(all="ignore"):
        want = x.astype(np.float32)
    got = np.array([ei.round_f32(Fraction(float(v))) for v in x], np.float32)
    assert np.array_equal(ei.bits(got)[x > 0], ei.bits(want)[x > 0])
    assert np.array_equal(ei.bits(got)[x < 0], ei.bits(want)[x < 0])
    assert np.isinf(got).sum() > 4 and (got == 0).sum() > 4 and ((got != 0) & (np.abs(got) < 2.0 ** -126)).sum() > 10
    assert _f32_bits(ei.round_f32(0)) == 0 and _f32_bits(ei.round_f32(Fraction(-1, 3))) == _f32_bits(np.float32(-1.0 / 3.0))


def test_round_f32_rounds_words_once():
    """2^63 + 2^39 + 1: exact 2^63 + 2^40, through a double 2^63.  And every word of the families against numpy's
    uint64 -> float32 cast (which rounds once here; the helper is the yardstick, the cast a witness)."""
    w = 2 ** 63 + 2 ** 39 + 1
    assert ei.frac(ei.round_f32(w)) == 2 ** 63 + 2 ** 40
    assert Fraction(float(np.float32(float(w)))) == 2 ** 63  # (through a double: rounded twice)
    words = np.array(ei.tie_words() + ei.double_rounding_words() + ei.TOP_BIT_WORDS + ei.SMALL_WORDS + ei.COUNT_WORDS, dtype=np.uint64)
    got = np.array([ei.round_f32(int(v)) for v in words], np.float32)
    assert np.array_equal(ei.bits(got), ei.bits(words.astype(np.float32)))
    twice = np.array([np.float32(float(int(v))) for v in words], np.float32)
    assert (ei.bits(twice) != ei.bits(got)).sum() >= 22  # the double_rounding words: a double gets every one of them wrong
    assert ei.frac(ei.round_f32(2 ** 64 - 1)) == 2 ** 64 and ei.frac(ei.round_f32(2 ** 64 - 2 ** 39 - 1)) == 2 ** 64 - 2 ** 40


# ---- resolve ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cornell(pkg):
    scene = pkg.Scene.cornell()
    yield scene
    scene.close()


def oracle_resolve(pkg, ob, scene, words, out):
    """the rows as a frame of one row through the oracle's own splat and out arrays"""
    orc = ob.OracleRender(pkg.abi, scene.desc, len(words), 1)
    orc.splat[:] = words
    orc.chan["out"][:] = out
    orc.resolve()
    got = orc.chan["out"].copy()
    orc.close()
    return got


def _resolve_f64_check(out, words, got):
    """(rows compared, the largest |got - float64| over its bound) on the rows whose `out` is finite and count is not 0"""
    ok = np.isfinite(out).all(axis=1) & (words[:, 3] != 0)
    want, bound = ei.resolve_f64(out[ok], words[ok])
    err = np.abs(got[ok].astype(np.float64) - want)
    assert (err <= bound).all(), f"{int((err > bound).sum())} values beyond the derived bound"
    return int(ok.sum())


@pytest.mark.parametrize("family", ei.WORD_FAMILIES)
def test_resolve_oracle_equals_exact(pkg, ob, cornell, family):
    words, out = ei.word_family(family)
    got = oracle_resolve(pkg, ob, cornell, words, out)
    want = ei.resolve_exact(out, words)
    differ = (ei.bits(got) != ei.bits(want)).any(axis=1)
    assert not differ.any(), f"{family}: rows {np.flatnonzero(differ)[:8]} differ from the exact reading"
    untouched = words[:, 3] == 0
    assert np.array_equal(ei.bits(got[untouched]), ei.bits(out[untouched]))
    assert _resolve_f64_check(out, words, got) >= (0 if family == "out_values" else 12)
    # the family is what it says
    if family in ("ties", "double_rounding", "top_bit"):
        probe = (out < 0).any(axis=1)
        col = got[probe][out[probe] < 0]  # the probes' answers: 0 where the word went down, more where it went up
        assert (col == 0).sum() >= 3 and (col > 0).sum() >= 3
    if family == "counts":
        assert untouched.sum() >= 5 and (words[untouched, 0:3] != 0).all()
        assert ((got[:, 3] > 0) & (got[:, 3] < 1)).any() and (got[:, 3] == 1).any() and (got[~untouched, 3] == 0).any()
    if family == "out_values":
        assert np.isnan(out).any() and not np.isnan(got).any() and not (np.signbit(got) & (got == 0)).any()
    if family == "small":
        tiny = (out[:, 0] != 0) & (np.abs(out[:, 0]) < 1e-37)  # a subnormal or tiny `out` is absorbed: the sum is the splat's value
        assert tiny.sum() >= 8 and (got[tiny, 0:3] == ei.resolve_exact(np.zeros_like(out), words)[tiny, 0:3]).all()
        assert (got == 1).any() and (got[:, 0:3] == F(1.0 - 2.0 ** -24)).any()


def test_double_rounding_is_caught(pkg, ob):
    """the probe pixels tell a conversion through a double from the right one: all 22 words"""
    words, out = ei.word_family("double_rounding")
    want = ei.resolve_exact(out, words)
    twice = out.copy()
    for i in range(len(out)):
        for c in range(3):
            v = np.float32(float(int(words[i, c]))) * np.float32(2.0 ** -32)
            twice[i, c] = min(max(np.float32(out[i, c] + v), np.float32(0)), np.float32(1))
    rows = (ei.bits(twice[:, 0:3]) != ei.bits(want[:, 0:3])).any(axis=1)
    assert rows[1::2].sum() == 22  # (every word's probe row; the ties themselves round alike both ways)


# ---- accumulate -------------------------------------------------------------------------------------------------------
def oracle_accumulate(pkg, ob, last, cur, n, nmax):
    lib = ob.load_oracle(pkg.abi)
    a, b = np.ascontiguousarray(last, F).copy(), np.ascontiguousarray(cur, F).copy()
    lib.oracle_accumulate(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), n, nmax, len(a))
    assert np.array_equal(ei.bits(a), ei.bits(b))
    return a


def measure_accumulate(family, run=ei.accumulate_f32):
    worst = 0.0
    for last, cur, n, nmax in ei.acc_family(family):
        worst = max(worst, ei.acc_deviation(run(last, cur, n, nmax), ei.accumulate_f64(last, cur, n, nmax)))
    return worst


@pytest.mark.parametrize("family", ei.ACC_FAMILIES)
def test_accumulate_oracle_equals_float32_restatement(pkg, ob, family):
    for last, cur, n, nmax in ei.acc_family(family):
        got = oracle_accumulate(pkg, ob, last, cur, n, nmax)
        want = ei.accumulate_f32(last, cur, n, nmax)
        assert ei.same_bits(got, want), (family, n, nmax)
        if not n < nmax:
            assert np.array_equal(ei.bits(got), ei.bits(last))


@pytest.mark.parametrize("family", ei.ACC_WELL)
def test_accumulate_within_measured_bound_of_float64(pkg, ob, family):
    measured = measure_accumulate(family, lambda *a: oracle_accumulate(pkg, ob, *a))
    print(f"accumulate {family}: measured {measured:.3e}, table {ei.MEASURED['accumulate ' + family]:.3e}")
    assert measured <= ei.bound_of(ei.MEASURED["accumulate " + family])
    assert measured >= 0.25 * ei.MEASURED["accumulate " + family]  # (the table is this measurement, not a loose guess)


@pytest.mark.parametrize("family", ["huge", "specials", "cancel"])
def test_accumulate_classes(pkg, ob, family):
    seen = set()
    for last, cur, n, nmax in ei.acc_family(family):
        got = ei.value_class(oracle_accumulate(pkg, ob, last, cur, n, nmax))
        want = ei.accumulate_class(last, cur, n, nmax)
        assert np.array_equal(got, want), (family, n, nmax)
        seen |= set(np.unique(got).tolist())
    need = {"huge": {1, 2, 6}, "specials": {0, 1, 2, 3, 4, 6}, "cancel": {0, 1, 5}}[family]
    assert need <= seen, (family, seen)


# ---- the adaptive update ----------------------------------------------------------------------------------------------
class Sequence:
    """one family's K frames through np_update and update_f64, and what the comparison of the two gives"""

    def __init__(self, family):
        W, H = SEQ_SHAPE
        P = ei.SEQ_PARAMS
        self.family, self.frames = family, ei.sequence_frames(family, W, H)
        self.steps = ei.run_sequence(self.frames)
        self.ref = ei.update_f64(self.frames, [s["mask_in"] for s in self.steps], P["threshold"], P["epsilon"], P["mn"], P["mx"])
        thr = float(F(P["threshold"]))
        scale = float(np.abs(self.frames).max())
        band = ei.MARGIN[family] * thr + 10.0 * ei.MEASURED["sequence " + family]["rel_abs"]
        self.dev_mean = self.dev_rel = self.dev_abs = 0.0
        self.margin = self.nan = self.of = self.differ = 0
        before = np.zeros(self.frames.shape[1:3], np.uint32)
        for s, (mean64, rel64, n64, conv64) in zip(self.steps, self.ref):
            assert np.array_equal(s["count"], n64)
            folded, before = s["count"] != before, s["count"]  # a pixel-update: the pixel took this frame in
            seen = n64 >= 1
            self.dev_mean = max(self.dev_mean, float(np.abs(s["mean"][seen] - mean64[seen]).max()) / scale)
            rel32 = s["rel"].astype(np.float64)
            both = (n64 >= P["mn"]) & np.isfinite(rel32) & np.isfinite(rel64)  # (below minSamples nothing reads the quotient)
            hi, lo = both & (rel64 > 1e-6), both & ~(rel64 > 1e-6)
            if hi.any():
                self.dev_rel = max(self.dev_rel, float((np.abs(rel32 - rel64)[hi] / rel64[hi]).max()))
            if lo.any():
                self.dev_abs = max(self.dev_abs, float(np.abs(rel32 - rel64)[lo].max()))
            live = folded & (n64 >= P["mn"])  # (a pixel that rests repeats its last decision: counted once)
            conv32 = (s["count"] >= P["mx"]) | (live & (s["rel"] <= F(P["threshold"])))
            nan = live & ~np.isfinite(rel32) & np.isfinite(rel64)
            inside = live & ~nan & ~(np.abs(rel64 - thr) > band)
            self.of += int(live.sum())
            self.nan += int(nan.sum())
            self.margin += int(inside.sum())
            self.differ += int((live & ~nan & ~inside & (conv32 != conv64)).sum())

    def left_out(self):
        return {"margin": self.margin, "nan": self.nan, "of": self.of}


_sequences = {}


def sequence(family):
    if family not in _sequences:
        _sequences[family] = Sequence(family)
    return _sequences[family]


@pytest.mark.parametrize("family", ei.SEQ_FAMILIES)
def test_update_against_float64_statistic(family):
    s = sequence(family)
    tab = ei.MEASURED["sequence " + family]
    print(f"sequence {family}: mean {s.dev_mean:.3e} (table {tab['mean']:.3e}), rel {s.dev_rel:.3e} (table {tab['rel']:.3e}), "
          f"rel_abs {s.dev_abs:.3e} (table {tab['rel_abs']:.3e}), left out {s.left_out()}, decisions that differ outside the margin {s.differ}")
    assert s.dev_mean <= ei.bound_of(tab["mean"]) and s.dev_rel <= ei.bound_of(tab["rel"]) and s.dev_abs <= ei.bound_of(tab["rel_abs"])
    assert s.dev_mean >= 0.25 * tab["mean"] and s.dev_rel >= 0.25 * tab["rel"] and s.dev_abs >= 0.25 * tab["rel_abs"]
    assert s.differ == 0, f"{s.differ} decisions differ from the float64 decision outside the margin"
    assert s.left_out() == ei.LEFT_OUT[family]
    allowed = WELL_LEFT_OUT if family in ei.SEQ_WELL else ILL_LEFT_OUT
    assert s.margin + s.nan <= allowed * s.of and s.of >= SEQ_SHAPE[0] * SEQ_SHAPE[1]  # every pixel decides at least once
    if family in ei.SEQ_WELL:
        assert s.nan == 0


@pytest.mark.parametrize("family", ei.SEQ_FAMILIES)
def test_sequence_properties(family):
    """`active` is the mask's sum and never grows; a pixel whose mask stayed 1 carries bdpt_accumulate's chain bit for bit;
    a pixel whose mask is 0 never changes again."""
    s = sequence(family)
    H, W = s.frames.shape[1:3]
    chain = np.zeros((H, W, 4), F)
    always = np.ones((H, W), bool)
    active = [W * H]
    for k, st in enumerate(s.steps):
        assert st["active"] == int(st["mask"].sum()) and set(np.unique(st["mask"]).tolist()) <= {0, 1}
        active.append(st["active"])
        always &= st["mask_in"] != 0
        chain = ei.accumulate_f32(chain, s.frames[k], k, 2 ** 32 - 1)
        assert np.array_equal(ei.bits(st["mean"][always]), ei.bits(chain[always])), k
        assert (st["count"][always] == k + 1).all()
        if k:
            off = st["mask_in"] == 0
            assert (st["mask"][off] == 0).all()
            for key in ("mean", "m2", "count"):
                assert np.array_equal(st[key][off], s.steps[k - 1][key][off]) or np.isnan(st[key][off]).any()
    assert all(b <= a for a, b in zip(active, active[1:])), active
    assert active[-1] < W * H, "nothing ever converged"
    if family == "ordinary":
        assert len(set(active)) > 8 and always.any()  # pixels converge at many counts, and some never do


def at_threshold_check():
    """the `solved` variant of at_threshold against the float64 reading of the same state's quotient"""
    W, H = SEQ_SHAPE
    label, st, P = ei.adaptive_states("at_threshold", W, H)[0]
    assert label == "solved" and not st["mask"].any()
    rel32 = ei.np_rel(st["mean"], st["m2"], st["count"], P["epsilon"])
    nf = st["count"].astype(np.float64)
    rel64 = np.sqrt(st["m2"].astype(np.float64) / (nf * (nf - 1))) / (ei.lum64(st["mean"]) + float(F(P["epsilon"])))
    thr = float(F(P["threshold"]))
    dev = float((np.abs(rel32 - rel64) / np.maximum(rel64, 1e-6)).max())
    inside = ~(np.abs(rel64 - thr) > ei.MARGIN["at_threshold"] * thr)
    differ = int((~inside & ((rel32 <= F(P["threshold"])) != (rel64 <= thr))).sum())
    exp = ei.np_update(st["mean"], st["m2"], st["count"], st["mask"], st["frame"], P["threshold"], P["epsilon"], P["mn"], P["mx"], 1)
    return st, rel32, dev, {"margin": int(inside.sum()), "nan": int((~np.isfinite(rel32)).sum()), "of": int(inside.size)}, differ, exp


def test_at_threshold_states():
    st, rel32, dev, left, differ, exp = at_threshold_check()
    tab = ei.MEASURED["state at_threshold"]["rel"]
    print(f"state at_threshold: rel {dev:.3e} (table {tab:.3e}), left out {left}, differ {differ}")
    assert dev <= ei.bound_of(tab) and dev >= 0.25 * tab
    assert differ == 0 and left == ei.LEFT_OUT["at_threshold"] and left["nan"] == 0
    assert left["margin"] <= ILL_LEFT_OUT * left["of"]
    # the family is what it says: quotients equal to the threshold (converged: <=), and the mask decides on either side
    solved = st["solved"]
    assert solved.sum() >= 100 and (rel32[solved] == F(0.2)).all() and (exp[3][solved] == 0).all()
    near = np.abs(rel32.astype(np.float64) / 0.2 - 1) < 1e-6
    assert (exp[3][near] == 1).sum() >= 100 and (exp[3][near] == 0).sum() >= 100


THRESHOLDS = {"threshold 0": lambda rel: rel <= 0, "threshold -0.0": lambda rel: rel <= 0, "threshold < 0": lambda rel: rel <= -1,
              "threshold inf": lambda rel: ~np.isnan(rel), "threshold NaN": lambda rel: np.zeros(rel.shape, bool)}


def test_rules_the_header_pins():
    """np_update on the points include/bdpt.h "Adaptive sampling" spells out: thresholds that are zero, negative, infinite or
    NaN; a denominator that is negative or zero; mask bytes other than 0 / 1; counts whose cast rounds."""
    W, H = SEQ_SHAPE
    for label, st, P in ei.adaptive_states("at_threshold", W, H)[1:]:
        mean, m2, count, mask, active, _ = ei.np_update(st["mean"], st["m2"], st["count"], st["mask"], st["frame"], P["threshold"],
                                                        P["epsilon"], P["mn"], P["mx"], 1)
        rel = ei.np_rel(mean, m2, count, P["epsilon"])
        conv = (count >= P["mx"]) | ((count >= P["mn"]) & THRESHOLDS[label](rel))
        assert np.array_equal(mask == 0, conv), label
        live = (count >= P["mn"]) & (count < P["mx"])
        if label in ("threshold < 0", "threshold NaN"):
            assert not conv[live].any() and live.sum() > 50, label  # never before maxSamples
        elif label == "threshold inf":
            assert conv[live & ~np.isnan(rel)].all() and live.sum() > 50, label
        else:
            assert conv[live].any() and not conv[live].all(), label  # m2 == 0 converges, the rest does not
    for label, st, P in ei.adaptive_states("negative", W, H):
        mean, m2, count, mask, active, _ = ei.np_update(st["mean"], st["m2"], st["count"], st["mask"], st["frame"], P["threshold"],
                                                        P["epsilon"], P["mn"], P["mx"], 1)
        den = ei._lum(mean) + F(P["epsilon"])
        live = (count >= P["mn"]) & (count < P["mx"])
        if label == "lum + eps < 0":
            assert (den < 0).all() and (mask[live & (m2 >= 0)] == 0).all() and live.sum() > 50  # -x <= threshold: converged
        else:
            zero = live & (den == 0)
            assert zero.sum() > 20 and (mask[zero & (m2 > 0)] == 1).all() and (mask[zero & (m2 == 0)] == 1).all()  # inf, NaN
    (_, st, P), = ei.adaptive_states("mask_bytes", W, H)
    exp = ei.np_update(st["mean"], st["m2"], st["count"], st["mask"], st["frame"], P["threshold"], P["epsilon"], P["mn"], P["mx"], 1)
    as01 = ei.np_update(st["mean"], st["m2"], st["count"], (st["mask"] != 0).astype(np.uint8), st["frame"], P["threshold"], P["epsilon"],
                        P["mn"], P["mx"], 1)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(exp[:4], as01[:4])) and set(np.unique(exp[3]).tolist()) == {0, 1}
    for label, st, P in ei.adaptive_states("counts", W, H):
        exp = ei.np_update(st["mean"], st["m2"], st["count"], st["mask"], st["frame"], P["threshold"], P["epsilon"], P["mn"], P["mx"], 1)
        upd = (st["mask"] != 0) & (st["count"] < P["mx"])
        assert np.array_equal(exp[2], st["count"] + upd.astype(np.uint32)), label
        assert (exp[3][exp[2] >= P["mx"]] == 0).all() and (exp[3][exp[2] < P["mn"]] == 1).all(), label
        at = upd & (st["count"] == 2 ** 24 + 1)
        if at.any():  # a = 2^24 (rounded down), b = 2^24 + 2: the mean moves by (c - mean) / b up to rounding, it does not jump
            assert np.abs(exp[0][at] - st["mean"][at]).max() < 1e-6


if __name__ == "__main__":
    print("MEASURED = {")
    for fam in ei.ACC_WELL:
        print(f'    "accumulate {fam}": {measure_accumulate(fam):.1e},')
    seqs = {fam: sequence(fam) for fam in ei.SEQ_FAMILIES}
    for fam, sq in seqs.items():
        print(f'    "sequence {fam}": {{"mean": {sq.dev_mean:.1e}, "rel": {sq.dev_rel:.1e}, "rel_abs": {sq.dev_abs:.1e}}},')
    chk = at_threshold_check()
    print(f'    "state at_threshold": {{"rel": {chk[2]:.1e}}},')
    print("}")
    print("MARGIN =", {k: float(f"{v:.1e}") for k, v in ei.MARGIN.items()}, " # (from the table in the module: run again after editing it)")
    print("LEFT_OUT = {")
    for fam, sq in seqs.items():
        print(f'    "{fam}": {sq.left_out()},  # decisions that differ outside the margin: {sq.differ}')
    print(f'    "at_threshold": {chk[3]},  # decisions that differ outside the margin: {chk[4]}')
    print("}")
