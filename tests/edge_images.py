"""Edge-case images for the tail of a frame (tests/test_edge_images_cpu.py, tests/test_gpu_edge_images.py): splat words
and `out` pixels for bdpt_resolve, frame pairs and counts for bdpt_accumulate, states, frames and frame sequences for
bdpt_adaptive_update — and the readings they are compared with.  Seeded, plain numpy, no product code.

Readings
  round_f32          one round-to-nearest-even of a Fraction to float32, done in integers: the yardstick of the word
                     conversion (np.float32(int(w)) goes through a double and rounds twice)
  resolve_exact      include/bdpt.h "bdpt_resolve" in exact arithmetic, each fp32 step rounded once by round_f32
  accumulate_f32/64  the running mean, step by step in float32 / the same expression in float64
  np_update          include/bdpt.h "Adaptive sampling", restated in float32 (what the kernel must equal bit for bit)
  update_f64         a float64 mean and a two-pass sample variance of the luminances of the frames folded in so far

MEASURED holds the worst deviation of the fp32 restatements from the float64 readings per family, MARGIN the band around
the threshold inside which a decision is not compared, LEFT_OUT what that band (and a NaN quotient) leaves out.  All three
are printed by `python tests/test_edge_images_cpu.py` and asserted by the tests."""
from fractions import Fraction

import numpy as np

F = np.float32
U64 = np.uint64
INV_FIX = Fraction(1, 2 ** 32)
SENTINEL = F(7.0)  # (a value no kernel here writes: every result is saturated, a mean of inputs, or an input)


def keeps_subnormals():
    """numpy keeps float32 subnormals in this process (a library that sets flush-to-zero would make every restatement here
    answer for another arithmetic than the header's)"""
    return bool(np.float32(1e-45) * np.float32(1) != 0) and bool(np.float32(1e-38) / np.float32(4) != 0)


def bound_of(measured):
    """four times the measured worst deviation, rounded up to one digit (edge_surfaces.bound_of)"""
    x = 4.0 * measured
    if x == 0:
        return 0.0
    e = np.floor(np.log10(x))
    return float(np.ceil(x / 10 ** e * (1 - 1e-12)) * 10 ** e)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    """bit for bit, but for a NaN's sign and payload: an invalid operation gives 0xFFC00000 on x86 and 0x7FC00000 on the
    GPU, and the header promises a NaN, not which one"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def value_class(a):
    """0 zero, 1 finite, 2 inf, 3 NaN — plus 4 for a set sign bit of anything but a NaN (edge_poses.value_class)"""
    a = np.asarray(a)
    c = np.where(np.isnan(a), 3, np.where(np.isinf(a), 2, np.where(a == 0, 0, 1)))
    return c + np.where(np.isnan(a), 0, 4 * np.signbit(a))


# ---- readings: the word conversion and the resolve --------------------------------------------------------------------
def round_f32(q):
    """The float32 nearest to the rational q, ties to even, as the hardware rounds: subnormals below 2^-126, inf from
    2^128 - 2^103 on.  Integer arithmetic only (no Python float in between).  A zero is +0.0."""
    q = Fraction(q)
    if q == 0:
        return F(0.0)
    sign = 0x80000000 if q < 0 else 0
    n, d = abs(q.numerator), q.denominator
    e = n.bit_length() - d.bit_length()  # 2^(e-1) < q < 2^(e+1)
    if (n << max(-e, 0)) < (d << max(e, 0)):
        e -= 1  # 2^e <= q < 2^(e+1)
    e = max(e, -126)  # (below: the subnormals' fixed spacing of 2^-149)
    sh = e - 23
    num, den = (n << -sh, d) if sh < 0 else (n, d << sh)
    m, r = divmod(num, den)
    if 2 * r > den or (2 * r == den and (m & 1)):
        m += 1
    if m == 1 << 24:
        m, e = m >> 1, e + 1
    if e > 127:
        word = 0x7F800000
    elif m < (1 << 23):
        word = m
    else:
        word = ((e + 127) << 23) | (m - (1 << 23))
    return np.array([sign | word], np.uint32).view(np.float32)[0]


def frac(x):
    """the exact value of a finite float32"""
    return Fraction(float(x))  # (float32 -> double is exact, and Fraction(double) is exact)


def _saturate(x):
    """device_math.hpp saturate: NaN and everything <= 0 (-0.0 too) -> +0.0, everything >= 1 -> 1"""
    y = x if x > 0 else F(0.0)
    return y if y < 1 else F(1.0)


def _add_saturate(o, v):
    """saturate(o + v) for a float32 o of any kind and a finite float32 v >= 0"""
    if np.isnan(o):
        return F(0.0)
    if np.isinf(o):
        return F(1.0) if o > 0 else F(0.0)
    return _saturate(round_f32(frac(o) + frac(v)))


def resolve_exact(out, words):
    """bdpt_resolve on (n, 4) float32 pixels and (n, 4) uint64 words, in exact arithmetic:
      v     = round_f32(word) * 2^-32       (exact: a power of two, and no word is small enough to underflow)
      out.c = saturate(round_f32(out.c + v))
      out.w = saturate(round_f32(out.w + round_f32(count)))
    and a pixel whose count word is 0 stays as it is."""
    out = np.array(out, np.float32)
    for i in range(len(out)):
        if int(words[i, 3]) == 0:
            continue
        for c in range(3):
            v = round_f32(frac(round_f32(int(words[i, c]))) * INV_FIX) if int(words[i, c]) else F(0.0)
            out[i, c] = _add_saturate(out[i, c], v)
        out[i, 3] = _add_saturate(out[i, 3], round_f32(int(words[i, 3])))
    return out


def resolve_f64(out, words):
    """the plain float64 value clip(out + word / 2^32, 0, 1), and the bound 2^-24 * (v + |out + v|) of the fp32 steps before
    the clamp (one rounding of the word, relative 2^-24 of v; one of the sum, relative 2^-24 of it; the scaling is exact).
    The clamp is monotonic and 1-Lipschitz, so it does not enlarge the bound.  Alpha adds the count itself."""
    o = np.asarray(out, np.float64)
    v = words.astype(np.float64)  # (uint64 -> double rounds by 2^-53 relative: far below the bound)
    v[:, 0:3] *= 2.0 ** -32
    with np.errstate(all="ignore"):
        s = o + v
        return np.clip(s, 0.0, 1.0), 2.0 ** -24 * (v + np.abs(s)) * (1 + 2.0 ** -20)


# ---- splat-word families ----------------------------------------------------------------------------------------------
WORD_FAMILIES = ("ordinary", "ties", "double_rounding", "top_bit", "small", "counts", "out_values")


def _lower_f32(w):
    """the largest float32 value <= the integer w (w truncated to 24 significant bits), as an integer"""
    w = int(w)
    s = max(w.bit_length() - 24, 0)
    return (w >> s) << s


def _word_rows(values, rng):
    """Rows that show how each word of `values` was rounded: the word in one colour channel (the channel rotates), ordinary
    words in the others, count 1.  Every word gets two pixels: an `out` in [0, 1), where a frame would have it, and
    -(the float32 just below the word) * 2^-32, which leaves the rounding of the word alone in the sum: 0 when it went down,
    one ulp of the word (saturated at 1) when it went up."""
    words, out = [], []
    for i, w in enumerate(values):
        for probe in (False, True):
            row = [int(x) for x in rng.integers(0, 2 ** 32, 3)] + [1]
            px = rng.random(4).astype(F)
            row[i % 3] = int(w)
            if probe:
                px[i % 3] = -round_f32(Fraction(_lower_f32(w)) * INV_FIX)
            words.append(row)
            out.append(px)
    return np.array(words, dtype=U64), np.array(out, F)


def tie_words():
    v = []
    for k in range(40):
        for base in ((2 ** 24 + 1) << k, (2 ** 24 + 3) << k):  # (ties that go down to even and up to even)
            v += [base - 1, base, base + 1]
    return v


def double_rounding_words():
    """Above a float32 tie by less than half a double ulp (a double sees the tie, and ties-to-even takes it down: the
    right answer is up), below one by as little (the double's tie goes up: the right answer is down), and the ties."""
    v = []
    for p in range(53, 64):  # the top bit
        s = p - 24
        v += [((2 ** 24 + 1) << s) + 1, ((2 ** 24 + 1) << s), ((2 ** 24 + 3) << s) - 1, ((2 ** 24 + 3) << s)]
    return v


TOP_BIT_WORDS = [2 ** 63 - 1, 2 ** 63, 2 ** 63 + 1, 2 ** 64 - 2 ** 39, 2 ** 64 - 2 ** 39 - 1, 2 ** 64 - 1]
SMALL_WORDS = [1, 2, 3, 2 ** 8, 2 ** 9 - 1]
SMALL_OUT = [0.0, -0.0, 1e-45, 1e-38, 1.0 - 2.0 ** -24]
COUNT_WORDS = [0, 1, 2, 2 ** 24 + 1, 2 ** 32, 2 ** 64 - 1]
OUT_VALUES = [np.nan, np.inf, -np.inf, -1.0, -0.0, 2.0, 1.0 - 2.0 ** -24, 1.0]


def word_family(name, seed=1):
    """(words (n, 4) uint64, out (n, 4) float32) of one family"""
    rng = np.random.default_rng([seed, WORD_FAMILIES.index(name)])
    if name == "ordinary":
        n = 96
        words = rng.integers(0, 8 * 2 ** 32 + 1, (n, 4)).astype(U64)
        words[:, 3] = rng.integers(1, 9, n)
        words[::7, 0:3] = 0
        return words, rng.random((n, 4)).astype(F)
    if name == "ties":
        return _word_rows(tie_words(), rng)
    if name == "double_rounding":
        return _word_rows(double_rounding_words(), rng)
    if name == "top_bit":
        return _word_rows(TOP_BIT_WORDS, rng)
    if name == "small":  # every word against every `out`, in every colour channel
        words, out = [], []
        for i, (w, o) in enumerate((w, o) for w in SMALL_WORDS for o in SMALL_OUT):
            row, px = [w, w, w, 1], np.full(4, o, F)
            row[i % 3] = SMALL_WORDS[(i + 1) % 5]  # (and a mixture, so that the channels are told apart)
            words.append(row)
            out.append(px)
        return np.array(words, dtype=U64), np.array(out, F)
    if name == "counts":
        words, out = [], []
        for cnt in [0] * 3 + COUNT_WORDS:  # (count 0 four times over: untouched pixels for every tile shape)
            for ow in (0.0, 0.25, -float(round_f32(_lower_f32(cnt))), -1.0, SENTINEL):
                words.append([int(x) for x in rng.integers(1, 2 ** 31, 3)] + [cnt])  # colour words never 0
                out.append(np.array([rng.random() * 0.5, rng.random() * 0.5, rng.random() * 0.5, ow], F))
        return np.array(words, dtype=U64), np.array(out, F)
    assert name == "out_values"
    words, out = [], []
    for o in OUT_VALUES:
        for w in (0, 1, 2 ** 31):
            for ch in range(4):  # the value in one channel, an ordinary one in the others
                px = rng.random(4).astype(F) * F(0.5)
                px[ch] = o
                words.append([w, w, w, 1])
                out.append(px)
        words.append([0, 1, 2 ** 31, 1])
        out.append(np.full(4, o, F))
    return np.array(words, dtype=U64), np.array(out, F)


_word_rows_cache = {}


def all_word_rows(seed=1):
    """(words, out, family label per row, exact result): every family, concatenated; computed once and shared"""
    if seed not in _word_rows_cache:
        fam = [word_family(k, seed) for k in WORD_FAMILIES]
        words = np.concatenate([f[0] for f in fam])
        out = np.concatenate([f[1] for f in fam])
        label = np.concatenate([np.full(len(f[0]), i, np.int32) for i, f in enumerate(fam)])
        exact = resolve_exact(out, words)
        for a in (words, out, label, exact):
            a.setflags(write=False)
        _word_rows_cache[seed] = (words, out, label, exact)
    return _word_rows_cache[seed]


def deal(nrows, npix, seed=3):
    """a row for every pixel: whole permutations of the rows, one after the other, so that any run of nrows pixels holds
    every row (and a tile of more pixels than that every family)"""
    rng = np.random.default_rng(seed)
    reps = (npix + nrows - 1) // nrows
    return np.concatenate([rng.permutation(nrows) for _ in range(reps)])[:npix]


# ---- the running mean -------------------------------------------------------------------------------------------------
def accumulate_f32(last, cur, n, nmax):
    """accumulate.ps.hlsl:28-42 as include/bdpt.h states it, one float32 operation at a time"""
    last, cur = np.asarray(last, F), np.asarray(cur, F)
    if not n < nmax:
        return last.copy()
    a, b = np.uint32(n).astype(F), np.uint32(n + 1).astype(F)  # (the casts round from 2^24 + 1 on)
    with np.errstate(all="ignore"):
        return ((a * last + cur) / b).astype(F)


def accumulate_f64(last, cur, n, nmax):
    """the same expression in float64 with the counts as they are"""
    last, cur = np.asarray(last, np.float64), np.asarray(cur, np.float64)
    if not n < nmax:
        return last.copy()
    with np.errstate(all="ignore"):
        return (float(n) * last + cur) / float(n + 1)


def accumulate_class(last, cur, n, nmax):
    """The class (value_class) of the running mean read in float64 with float32's range: each of the three steps a * last,
    + cur, / b is made in float64 and overflows to an infinity where float32 would (beyond its largest finite value; a
    float64 alone would keep 2 * 3e38 finite).  Underflow cannot change a class here: the families that use this reading
    (huge, specials, cancel) have no result below 2^-126 that is not an exact zero."""
    fmax = float(np.finfo(np.float32).max)
    last, cur = np.asarray(last, np.float64), np.asarray(cur, np.float64)
    if not n < nmax:
        return value_class(last)

    def rng32(x):
        return np.where(np.abs(x) > fmax, np.copysign(np.inf, x), x)

    with np.errstate(all="ignore"):
        return value_class(rng32(rng32(rng32(float(np.uint32(n).astype(F)) * last) + cur) / float(np.uint32(n + 1).astype(F))))


ACC_FAMILIES = ("ordinary", "counts", "subnormal", "huge", "specials", "cancel")
ACC_WELL = ("ordinary", "counts", "subnormal")
ACC_COUNTS = [(0, 2 ** 32 - 1), (1, 2 ** 32 - 1), (2 ** 24 - 1, 2 ** 32 - 1), (2 ** 24, 2 ** 32 - 1), (2 ** 24 + 1, 2 ** 32 - 1),
              (2 ** 31, 2 ** 32 - 1), (2 ** 32 - 2, 2 ** 32 - 1), (2 ** 32 - 1, 2 ** 32 - 1), (100, 100), (101, 100), (5, 0)]


def _step(x, k):
    """x moved k float32 values up (k < 0: down)"""
    x = np.asarray(x, F).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf if k > 0 else -np.inf))
    return x


def acc_family(name, seed=2):
    """a list of cases (last (m, 4), cur (m, 4), accumCount, maxAccumCount)"""
    rng = np.random.default_rng([seed, ACC_FAMILIES.index(name)])
    m = 64
    uni = lambda: rng.uniform(0, 2, (m, 4)).astype(F)  # noqa: E731  (test_accumulate_matches_oracle's values)
    if name == "ordinary":
        return [(uni(), uni(), n, 100) for n in range(5)]
    if name == "counts":
        return [(uni(), uni(), n, nmax) for n, nmax in ACC_COUNTS]
    if name == "subnormal":  # inputs from 1e-45 to 1e-38, either sign: products, sums and quotients around the subnormals
        val = lambda: (10.0 ** rng.uniform(-45, -38, (m, 4)) * rng.choice([-1.0, 1.0], (m, 4))).astype(F)  # noqa: E731
        return [(val(), val(), n, 100) for n in (0, 1, 3, 7)]
    if name == "huge":
        big = lambda: (rng.uniform(1.0, 3.4, (m, 4)) * 1e38 * rng.choice([-1.0, 1.0], (m, 4))).astype(F)  # noqa: E731
        three = np.full((m, 4), 3e38, F)
        return [(three, three, 1, 100), (three, three, 2, 100), (three, -three, 1, 100), (big(), big(), 1, 100), (big(), big(), 3, 100),
                (big(), uni(), 2, 100), (uni(), big(), 2, 100)]
    if name == "specials":
        s = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, -2.5], F)
        last, cur = np.meshgrid(s, s, indexing="ij")
        pad = (-last.size) % 4
        last = np.concatenate([last.ravel(), np.ones(pad, F)]).reshape(-1, 4)
        cur = np.concatenate([cur.ravel(), np.ones(pad, F)]).reshape(-1, 4)
        return [(last, cur, n, nmax) for n, nmax in ((0, 100), (1, 100), (3, 100), (100, 100), (0, 0))]
    assert name == "cancel"
    # `last` on a grid of 2^-12, so that a * last is exact in float32 (a <= 7) and both readings cancel to the same zero
    cases = []
    for n in (1, 3, 7):
        last = (rng.integers(1, 2 ** 13, (m, 4)) * 2.0 ** -12 * rng.choice([-1.0, 1.0], (m, 4))).astype(F)
        cur = (-F(n) * last).astype(F)
        for k in (0, 1, -1):
            cases.append((last, _step(cur, k), n, 100))
    return cases


def acc_deviation(got, want64):
    """the largest |got - want64| over max(|want64|, the smallest normal float32): relative, with the subnormals' fixed
    spacing counted against the smallest normal"""
    tiny = float(np.finfo(np.float32).tiny)
    with np.errstate(all="ignore"):
        return float((np.abs(np.asarray(got, np.float64) - want64) / np.maximum(np.abs(want64), tiny)).max())


# ---- the adaptive update ----------------------------------------------------------------------------------------------
def _lum(v):
    return (F(0.2126) * v[..., 0] + F(0.7152) * v[..., 1]) + F(0.0722) * v[..., 2]


def np_update(mean, m2, count, mask, frame, threshold, epsilon, mn, mx, B):
    """include/bdpt.h "Adaptive sampling", restated in float32."""
    H, W = count.shape
    upd = (mask != 0) & (count < mx)
    with np.errstate(all="ignore"):
        a = count.astype(F)[..., None]
        b = (count + 1).astype(F)[..., None]
        new = (a * mean + frame) / b
        lc, lo, ln = _lum(frame), _lum(mean), _lum(new)
        m2n = m2 + (lc - lo) * (lc - ln)
    mean = np.where(upd[..., None], new, mean).astype(F)
    m2 = np.where(upd, m2n, m2).astype(F)
    count = np.where(upd, count + 1, count).astype(np.uint32)
    nf = count.astype(F)
    with np.errstate(all="ignore"):
        rel = np.sqrt(m2 / (nf * (nf - F(1.0)))) / (_lum(mean) + F(epsilon))
    conv = (count >= mx) | ((count >= mn) & (rel <= F(threshold)))
    Hb, Wb = (H + B - 1) // B, (W + B - 1) // B
    unc = np.zeros((Hb * B, Wb * B), bool)
    unc[:H, :W] = ~conv
    blk = unc.reshape(Hb, B, Wb, B).any(axis=(1, 3))
    newmask = np.kron(blk, np.ones((B, B), bool))[:H, :W].astype(np.uint8)
    return mean, m2, count, newmask, int(newmask.sum()), mean.copy()


def np_rel(mean, m2, count, epsilon):
    """the quotient np_update compares with the threshold"""
    nf = count.astype(F)
    with np.errstate(all="ignore"):
        return np.sqrt(m2 / (nf * (nf - F(1.0)))) / (_lum(mean) + F(epsilon))


def lum64(v):
    v = np.asarray(v, np.float64)
    return 0.2126 * v[..., 0] + 0.7152 * v[..., 1] + 0.0722 * v[..., 2]


def update_f64(frames, masks, threshold, epsilon, mn, mx):
    """The statistic the update estimates, in float64: frames (K, H, W, 4), masks (K, H, W) the mask each frame was
    rendered with.  Frame k is folded into a pixel when its mask is set and fewer than mx frames are in.  Per step:
    (mean (H, W, 4), rel (H, W), n (H, W), converged (H, W)) with a two-pass sample variance of the folded frames'
    luminances and rel = sqrt(var / n) / (lum(mean) + epsilon)."""
    frames = np.asarray(frames, np.float64)
    K = len(frames)
    lums = lum64(frames)
    folded = np.zeros(lums.shape, bool)
    n = np.zeros(lums.shape[1:], np.int64)
    steps = []
    for k in range(K):
        folded[k] = (np.asarray(masks[k]) != 0) & (n < mx)
        n = n + folded[k]
        w = folded[:k + 1].astype(np.float64)
        with np.errstate(all="ignore"):
            mean = (w[..., None] * frames[:k + 1]).sum(0) / n[..., None]
            lbar = (w * lums[:k + 1]).sum(0) / n
            var = (w * (lums[:k + 1] - lbar) ** 2).sum(0) / (n - 1)
            rel = np.sqrt(var / n) / (lum64(mean) + float(F(epsilon)))
            conv = (n >= mx) | ((n >= mn) & (rel <= float(F(threshold))))
        steps.append((mean, rel, n.copy(), conv))
    return steps


SHAPES = ((1, 1), (1, 17), (17, 1), (8, 8), (9, 9), (16, 16), (17, 17), (15, 33), (67, 45))  # W x H
WIDE = (32785, 17)
BLOCKS = (1, 2, 4, 8, 16)
STATE_FAMILIES = ("ordinary", "dark", "bright_quiet", "hdr", "ulp_noise", "underflow", "black", "negative", "specials", "counts",
                  "mask_bytes", "at_threshold")
SEQ_FAMILIES = ("ordinary", "dark", "bright_quiet", "hdr", "ulp_noise")
SEQ_WELL = ("ordinary", "dark", "bright_quiet", "hdr")
SEQ_K = 32
SEQ_PARAMS = dict(threshold=0.05, epsilon=1e-3, mn=4, mx=40)  # (mx beyond K: every decision of a sequence is the quotient's)
SEQ_BLOCK = 2


def _colours(rng, H, W, level, spread):
    """RGBA float64 whose luminance is level * (1 +- spread) (uniform), alpha 1"""
    lum = level * (1.0 + spread * rng.uniform(-1, 1, (H, W)))
    tint = rng.uniform(0.7, 1.3, (H, W, 3))
    tint /= lum64(tint)[..., None]
    return np.concatenate([tint * lum[..., None], np.ones((H, W, 1))], axis=2)


def _base_state(rng, H, W, mn, mx, mean, frame, sigma_lum):
    """the existing recipe's counts, m2 and mask around a given mean and frame: counts 0 .. mx + 1 with a share at mn - 1,
    m2 = what `count` draws of luminance noise sigma_lum would have summed (30 % zero: converges at mn), a converged
    region on the left (whole blocks of every size turn inactive), a mask of 70 %"""
    count = rng.integers(0, mx + 2, (H, W)).astype(np.uint32)
    count[rng.random((H, W)) < 0.2] = mn - 1
    m2 = (rng.random((H, W)) * 2.0 * sigma_lum ** 2 * count).astype(F)
    m2[rng.random((H, W)) < 0.3] = 0.0
    count[:, :(W * 3) // 5] = mx
    mask = (rng.random((H, W)) < 0.7).astype(np.uint8)
    return dict(mean=np.ascontiguousarray(mean, F), m2=m2, count=count, mask=mask, frame=np.ascontiguousarray(frame, F))


LEVELS = {"dark": (None, 0.2), "bright_quiet": (0.9, 5e-4 / 0.9), "hdr": (1000.0, 0.5 / 1000.0), "ulp_noise": (1.0, 5e-7)}


def _level_images(rng, name, H, W, k=2):
    """k images of a family given by a luminance level and a relative noise: (base, noisy, noisy, ...)"""
    level, spread = LEVELS[name]
    if level is None:  # dark: luminances 1e-3 and 1e-6, in patches
        level = np.where(rng.random((H, W)) < 0.5, 1e-3, 1e-6)
    base = _colours(rng, H, W, level, 0.0)
    return [base] + [base * (1.0 + spread * rng.uniform(-1, 1, (H, W)))[..., None] for _ in range(k - 1)]


def _params(thr=0.2, eps=1e-3, mn=4, mx=9):
    return dict(threshold=thr, epsilon=eps, mn=mn, mx=mx)


def adaptive_states(name, W, H, seed=4):
    """a list of (label, state, params): state = dict(mean, m2, count, mask, frame) of an H x W frame"""
    rng = np.random.default_rng([seed, STATE_FAMILIES.index(name), W, H])
    P = _params()
    mn, mx = P["mn"], P["mx"]

    def ordinary():
        mean = rng.random((H, W, 4), dtype=F) * F(0.8)
        frame = (mean + (rng.random((H, W, 4), dtype=F) - F(0.5)) * F(0.3)).astype(F)
        return _base_state(rng, H, W, mn, mx, mean, frame, 0.16)

    if name == "ordinary":
        return [("", ordinary(), P)]
    if name in LEVELS:
        mean, frame = _level_images(rng, name, H, W)
        sig = LEVELS[name][1] * lum64(mean)
        st = _base_state(rng, H, W, mn, mx, mean, frame, 1.0)
        st["m2"] = (st["m2"].astype(np.float64) * sig ** 2).astype(F)
        return [("", st, _params(thr=0.05))]
    if name == "underflow":  # the deviation product (1e-20)^2 and below underflows; m2 holds subnormals and zeros
        out = []
        for eps in (0.0, 1e-3):
            level = 10.0 ** rng.uniform(-30, -20, (H, W))
            mean = _colours(rng, H, W, level, 0.0)
            frame = mean * (1.0 + 0.5 * rng.uniform(-1, 1, (H, W)))[..., None]
            st = _base_state(rng, H, W, mn, mx, mean, frame, 1.0)
            st["m2"] = np.where(rng.random((H, W)) < 0.5, F(1e-45), F(0.0)).astype(F) * (st["m2"] != 0)
            out.append((f"eps {eps}", st, _params(thr=0.05, eps=eps)))
        return out
    if name == "black":
        out = []
        for eps in (0.0, 1e-3):
            z = np.zeros((H, W, 4))
            st = _base_state(rng, H, W, mn, mx, z, z, 0.0)
            out.append((f"eps {eps}", st, _params(eps=eps)))
        return out
    if name == "negative":
        c0 = np.array([-0.5, -0.25, -0.125, 1.0], F)
        mean = np.tile(c0, (H, W, 1))
        frame = mean * (1.0 + 0.2 * rng.uniform(-1, 1, (H, W)))[..., None]
        out = []
        for label, eps in (("lum + eps < 0", 1e-3), ("lum + eps == 0", float(-_lum(c0)))):  # == 0 where the mask is 0
            st = _base_state(rng, H, W, mn, mx, mean, frame, 0.05)
            out.append((label, st, _params(eps=eps)))
        return out
    if name == "specials":
        st = ordinary()
        vals = np.array([np.nan, np.inf, -np.inf], F)
        for key, share in (("frame", 0.1), ("mean", 0.1)):
            hit = rng.random((H, W, 4)) < share
            st[key][hit] = rng.choice(vals, int(hit.sum()))
        hit = rng.random((H, W)) < 0.1
        st["m2"][hit] = rng.choice(vals, int(hit.sum()))
        hit = rng.random((H, W)) < 0.1
        st["m2"][hit] = -st["m2"][hit] - F(0.01)  # negative: a caller's state (sqrtf -> NaN: not converged)
        return [("", st, P)]
    if name == "counts":
        out = []
        for label, cmn, cmx, counts in (("max 9", 4, 9, [0, 1, 3, 4, 8, 9, 10]), ("min 2", 2, 9, [0, 1, 2, 8, 9, 10]),
                                        ("max 2^32 - 1", 2, 2 ** 32 - 1, [0, 1, 2, 2 ** 24, 2 ** 24 + 1, 2 ** 32 - 2, 2 ** 32 - 1]),
                                        ("max 2^24 + 1", 2, 2 ** 24 + 1, [2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 2])):
            st = ordinary()
            st["count"] = rng.choice(np.array(counts, np.uint32), (H, W))
            # m2 as large as the count makes it: about half of the pixels on either side of the threshold
            st["m2"] = (rng.random((H, W)) * 0.04 * st["count"].astype(np.float64) ** 2).astype(F)
            out.append((label, st, _params(mn=cmn, mx=cmx)))
        return out
    if name == "mask_bytes":
        st = ordinary()
        st["mask"] = rng.choice(np.array([0, 1, 2, 255], np.uint8), (H, W))
        return [("", st, P)]
    assert name == "at_threshold"
    out = []
    st = ordinary()
    st["count"] = rng.integers(mn, mx, (H, W)).astype(np.uint32)
    st["mask"][:] = 0  # nothing is folded in: the state that is tested is the state given
    thr, eps = F(0.2), F(1e-3)
    nf = st["count"].astype(np.float64)
    m2 = ((float(thr) * (lum64(st["mean"].astype(np.float64)) + float(eps))) ** 2 * nf * (nf - 1)).astype(F)
    solved = np.zeros((H, W), bool)
    for k in (0, 1, -1, 2, -2, 3, -3):  # the float32 quotient equals the threshold for some m2 next to the real solution
        cand = _step(m2, k)
        hit = ~solved & (np_rel(st["mean"], cand, st["count"], eps) == thr)
        m2 = np.where(hit, cand, m2)
        solved |= hit
    side = rng.integers(-1, 2, (H, W))  # one step of m2 below, at, above
    near = np.where(side == 0, m2, np.where(side > 0, _step(m2, 1), _step(m2, -1))).astype(F)
    # (and 60 % of the pixels well off the threshold, 0.1 % to 50 % of m2 either way: the float64 decision binds there)
    off = (m2 * (1.0 + rng.choice([-1.0, 1.0], (H, W)) * 10.0 ** rng.uniform(-3, np.log10(0.5), (H, W)))).astype(F)
    far = rng.random((H, W)) < 0.6
    st["m2"] = np.where(far, off, near)
    st["solved"] = solved & (side == 0) & ~far
    out.append(("solved", st, _params(thr=float(thr), eps=float(eps))))
    for label, t in (("threshold 0", 0.0), ("threshold -0.0", -0.0), ("threshold < 0", -1.0), ("threshold inf", np.inf),
                     ("threshold NaN", np.nan)):
        out.append((label, ordinary(), _params(thr=t)))
    return out


def sequence_frames(name, W, H, K=SEQ_K, seed=5):
    """K float32 frames of one of SEQ_FAMILIES: a fixed image plus fresh noise per frame.  `ordinary` gives every pixel a
    noise level of its own (3 % to 40 % of its luminance), so that pixels converge at every count."""
    rng = np.random.default_rng([seed, SEQ_FAMILIES.index(name), W, H])
    if name == "ordinary":
        base = _colours(rng, H, W, rng.uniform(0.1, 0.8, (H, W)), 0.0)
        spread = 10.0 ** rng.uniform(np.log10(0.03), np.log10(0.4), (H, W))
        return np.stack([base * (1.0 + spread * np.sqrt(3.0) * rng.uniform(-1, 1, (H, W)))[..., None] for _ in range(K)]).astype(F)
    return np.stack(_level_images(rng, name, H, W, K + 1)[1:]).astype(F)


def reset_state(H, W):
    return dict(mean=np.zeros((H, W, 4), F), m2=np.zeros((H, W), F), count=np.zeros((H, W), np.uint32), mask=np.ones((H, W), np.uint8))


def run_sequence(frames, P=SEQ_PARAMS, B=SEQ_BLOCK):
    """np_update from reset on over the frames, the mask fed back as the pipeline feeds it (a pixel whose mask is 0 is not
    rendered: its frame value is the mean it shows).  -> per step dict(mean, m2, count, mask_in, mask, active, rel)"""
    H, W = frames.shape[1:3]
    st = reset_state(H, W)
    steps = []
    for fr in frames:
        mask_in = st["mask"]
        shown = np.where((mask_in != 0)[..., None], fr, st["mean"]).astype(F)
        mean, m2, count, mask, active, _ = np_update(st["mean"], st["m2"], st["count"], mask_in, shown, P["threshold"], P["epsilon"],
                                                     P["mn"], P["mx"], B)
        st = dict(mean=mean, m2=m2, count=count, mask=mask)
        steps.append(dict(st, mask_in=mask_in, active=active, rel=np_rel(mean, m2, count, P["epsilon"])))
    return steps


# ---- measured tables (printed by `python tests/test_edge_images_cpu.py`) -----------------------------------------------
# accumulate: acc_deviation of accumulate_f32 (== oracle_accumulate == accumulate_kernel, bit for bit) from accumulate_f64.
# sequences (67 x 45, K = 32, SEQ_PARAMS, block 2), over all pixel-updates:
#   mean     the largest |mean32 - mean64| over the largest |value| of the family's frames (absolute deviation, on the
#            family's scale)
#   rel      the largest |rel32 - rel64| / rel64 where rel64 > 1e-6, both finite, count >= minSamples (below it nothing
#            reads the quotient; a pixel whose first two luminances nearly coincide has a variance of rounding noise there)
#   rel_abs  the largest |rel32 - rel64| where rel64 <= 1e-6 (ulp_noise lies there entirely: its m2 is rounding noise, so
#            a relative deviation of it means nothing)
MEASURED = {
    "accumulate ordinary": 9.1e-08,
    "accumulate counts": 1.4e-07,
    "accumulate subnormal": 7.5e-08,
    "sequence ordinary": {"mean": 2.9e-07, "rel": 1.4e-05, "rel_abs": 0.0e+00},
    "sequence dark": {"mean": 1.4e-07, "rel": 4.3e-06, "rel_abs": 0.0e+00},
    "sequence bright_quiet": {"mean": 1.0e-07, "rel": 2.2e-03, "rel_abs": 0.0e+00},
    "sequence hdr": {"mean": 9.7e-08, "rel": 1.7e-03, "rel_abs": 0.0e+00},
    "sequence ulp_noise": {"mean": 9.9e-08, "rel": 0.0e+00, "rel_abs": 8.3e-08},
    "state at_threshold": {"rel": 1.9e-07},  # the quotient of the given state, float32 against the same formula in float64
}
# ten times the worst relative deviation of rel measured for the family (MEASURED[...]["rel"]).  A decision is compared
# with the float64 decision where |rel64 - threshold| > MARGIN * threshold + 10 * rel_abs: the same factor on the absolute
# deviation of the quotients too small for a relative one.
MARGIN = {k.split()[1]: 10.0 * v["rel"] for k, v in MEASURED.items() if isinstance(v, dict)}
# pixel-updates (the pixel took the frame in, and its count has reached minSamples) whose decision is not compared: inside the margin, or with a NaN float32 quotient
# (m2 < 0 from rounding: "not converged" by the header's rule, whatever the float64 statistic says) — of `of` in all
LEFT_OUT = {
    "ordinary": {"margin": 7, "nan": 0, "of": 58173},
    "dark": {"margin": 0, "nan": 0, "of": 3023},  # (the quiet families converge at minSamples: one decision per pixel)
    "bright_quiet": {"margin": 0, "nan": 0, "of": 3015},
    "hdr": {"margin": 0, "nan": 0, "of": 3015},
    "ulp_noise": {"margin": 0, "nan": 1, "of": 3019},
    "at_threshold": {"margin": 1210, "nan": 0, "of": 3015},
}
