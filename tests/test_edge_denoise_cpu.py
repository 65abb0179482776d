"""The BMFR oracle (oracle/bmfr_oracle.cpp) against the float64 reading of the shaders (tests/bmfr_reference_numpy.py) on
the edge-case families of tests/edge_denoise.py: every family at every frame size, each stage alone, the two temporal
stages and all three, half and full frame, both QR variants.  Finite outputs within FIT_RTOL / TEMPORAL_RTOL of
test_bmfr_cross_check.py (the ill-conditioned families: within the bound measured for them), every output of the
reading's value class, accept bools and prev_frame_pixel_f exactly; the texels a decision margin leaves out are counted
and capped.  No GPU.  `python tests/test_edge_denoise_cpu.py` prints the tables edge_denoise.py records."""
import numpy as np
import pytest

import bmfr_reference_numpy as ref
import edge_denoise as ed

_tallies = {}


def family_tally(pkg, ob, family, W, H, sem=ref.D3D, only=None):
    """the oracle against the reading over every run and flag set of a family at one size (cached for the D3D reading)"""
    key = (family, W, H)
    if sem is ref.D3D and only is None and key in _tallies:
        return _tallies[key]
    tally = ed.Tally()
    for run, frames in ed.sequences(family, W, H).items():
        for label, flags in ed.flag_sets_of(family, run):
            if only is not None and not only(run, label):
                continue
            b, execute = ed.oracle_executor(pkg, ob, W, H)
            ed.run_sequence(tally, f"{family}/{run} {W}x{H} {label}", pkg, W, H, flags, frames, execute, sem, family in ed.ILL)
            b.close()
    if sem is ref.D3D and only is None:
        _tallies[key] = tally
    return tally


def within(tally, family):
    """the numeric bounds of a family: (fit ignore_ld, fit keep_ld, temporal) measured and allowed"""
    if family in ed.ILL:
        allowed = {k: 10.0 * v for k, v in ed.MEASURED[family]["fit"].items()}
        temporal = 10.0 * ed.MEASURED[family]["temporal"]
    else:
        allowed, temporal = ed.FIT_RTOL, ed.TEMPORAL_RTOL
    return [(tally.fit[False], allowed[False]), (tally.fit[True], allowed[True]), (tally.temporal, temporal)]


@pytest.mark.parametrize("W,H", ed.SIZES)
@pytest.mark.parametrize("family", list(ed.FAMILIES))
def test_oracle_matches_float64_reading(pkg, ob, family, W, H):
    tally = family_tally(pkg, ob, family, W, H)
    assert not tally.bad, tally.bad[:8]
    assert tally.classes > 0 and tally.written > 0
    for measured, allowed in within(tally, family):
        assert measured <= allowed, (family, within(tally, family), tally.worst)


@pytest.mark.parametrize("family", list(ed.FAMILIES))
def test_left_out_texels_stay_within_the_cap(pkg, ob, family):
    """what a decision margin leaves out is what edge_denoise.LEFT_OUT records, and at most 2 % of the processed texels"""
    total = ed.Tally()
    for W, H in ed.SIZES:
        total.merge(family_tally(pkg, ob, family, W, H))
    rec = ed.LEFT_OUT[family]
    assert total.written == rec["of"], (total.written, rec)
    assert total.left_out <= rec["left_out"], (total.left_out, rec)
    assert rec["left_out"] <= ed.CAP * rec["of"], rec


def test_families_reach_non_finite_results(pkg, ob):
    """non-finite results do occur, and are compared by class"""
    seen = 0
    for family in ("background", "non_finite", "albedo", "colour", "motion"):
        seen += family_tally(pkg, ob, family, 33, 31).nonfinite
    assert seen > 1000, seen


# ---- positive controls: the reading with another semantics must visibly miss ---------------------------------------------
def _misses(tally, family):
    return bool(tally.bad) or any(m > a for m, a in within(tally, family))


def test_reading_with_std_max_misses(pkg, ob):
    """std::max / std::min keep a NaN: the block range of a block with one NaN position (regressionCP.hlsl:133-175) and
    the blend_alpha clamps (preprocess.ps.hlsl:148, postprocess.ps.hlsl:81) come out as NaN"""
    sem = ref.Semantics(max_keeps_nan=True)
    t = family_tally(pkg, ob, "non_finite", 33, 31, sem, only=lambda run, label: label.startswith("fit/full"))
    assert _misses(t, "non_finite")
    t = family_tally(pkg, ob, "colour", 33, 31, sem, only=lambda run, label: label.startswith("switch_stages/full/ignore"))
    assert _misses(t, "colour")
    t = family_tally(pkg, ob, "albedo", 65, 33, sem, only=lambda run, label: label.startswith("all/full/ignore"))
    assert _misses(t, "albedo")


def test_reading_with_int_min_for_nan_misses(pkg, ob):
    """int(NaN) = INT_MIN (x86) tests no tap; D3D's 0 tests the taps around pixel (0,0) (preprocess.ps.hlsl:80)"""
    sem = ref.Semantics(int_of_nan=-2 ** 31)
    t = family_tally(pkg, ob, "background", 33, 31, sem, only=lambda run, label: run == "eye_at_origin" and label.startswith("pre/full"))
    assert any("accept" in b for b in t.bad), t.bad[:4]


def test_reading_with_unrounded_prev_pixel_misses(pkg, ob):
    """postprocess truncates what RG16Float holds of prev_frame_pixel_f (postprocess.ps.hlsl:41-42): 4 - 2^-11 is 4 there"""
    sem = ref.Semantics(round_prev_pixel=False)
    t = family_tally(pkg, ob, "borders", 33, 31, sem, only=lambda run, label: label.startswith("temporal/full"))
    assert _misses(t, "borders")


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as ge
    import oracle_binding
    package = ge.load_package()
    oracle_binding.load_oracle(package.abi)
    print("MEASURED = {")
    rows = []
    for fam in ed.FAMILIES:
        total = ed.Tally()
        for size in ed.SIZES:
            total.merge(family_tally(package, oracle_binding, fam, *size))
        print(f'    "{fam}": {{"fit": {{False: {total.fit[False]:.1e}, True: {total.fit[True]:.1e}}}, "temporal": {total.temporal:.1e}}},')
        rows.append(f'    "{fam}": {{"left_out": {total.left_out}, "of": {total.written}}},  # {total.causes} {100 * total.left_out / total.written:.2f} %')
        for line in total.bad[:6]:
            print("        #", line)
    print("}\nLEFT_OUT = {")
    print("\n".join(rows))
    print("}")
