"""Preconditions of tests/test_sinc_nt_gpu.py, verified without a GPU and with the oracle only: the NT set follows the tap-mode
table, every case holds the lanes it is named for, every oracle output is large enough for 1e-5 of its peak to mean something,
NaN footprints are the reference's window, the C oracle agrees with the numpy statement beyond the goldens' NT = 100, and the
float64 sum is well conditioned on the inputs chosen (an error found on the GPU is then the kernel's)."""
import numpy as np
import pytest

import sinc_nt_inputs as I
from test_sinc_tap_modes_cpu import ask_table, build_table_program

from oracle import oracle_c as C
from oracle import oracle_np


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return ask_table(build_table_program(tmp_path_factory.mktemp("sinc_nt_inputs")), list(range(1, 513)))


def chunk_forms(table, NT):
    """form of every chunk n0 = 1, 5, .. of the generic loops at this NT; the last entry is the LAST chunk's"""
    p1, p0 = table[NT]
    return ["rcp" if n0 == 1 else "taylor" if n0 < p1 else "linear" if n0 < p0 else "constant"
            for n0 in range(1, (NT - 1) // I.CHUNK * I.CHUNK + 2, I.CHUNK)]


def test_nt_set_follows_the_table(table):
    forms = {NT: chunk_forms(table, NT) for NT in range(1, 513)}
    assert min(NT for NT in forms if "linear" in forms[NT]) == I.NT_FIRST_LINEAR
    assert min(NT for NT in forms if "constant" in forms[NT]) == I.NT_FIRST_CONSTANT
    assert all(forms[NT] == ["rcp"] for NT in I.NT_SMALL) and forms[5] != ["rcp"]
    assert tuple(sorted(NT for NT in forms if forms[NT][-1] == "linear")) == tuple(sorted(I.NT_LAST_LINEAR))
    assert tuple(min(NT for NT in forms if forms[NT][-1] == "constant" and NT % 4 == r) for r in range(4)) == I.NT_LAST_CONSTANT
    assert sorted(NT for NT in forms if forms[NT][-1] == "taylor") == [7, 8]          # both among NT_TAYLOR
    # multi-chunk NT of every residue, so every mask pattern of a LAST chunk behind full ones
    assert {NT % 4 for NT in I.NT_SET if NT > 4} == {0, 1, 2, 3} and {NT % 4 for NT in I.NT_LARGE} == {0, 1, 2, 3}
    for group in (I.NT_SMALL, I.NT_TAYLOR, (I.NT_FIRST_LINEAR, I.NT_FIRST_CONSTANT), I.NT_LAST_LINEAR, I.NT_LAST_CONSTANT,
                  I.NT_NEXT_TO_SPECIALISED, I.NT_SPECIALISED, I.NT_LARGE, I.NT_FUSED_SPAN, I.NT_TOP, I.NT_NONFINITE, I.NT_FUSED):
        assert set(group) <= set(I.NT_SET)
    # the forms' boundaries move inside the set
    assert len({table[NT] for NT in I.NT_SET}) >= 15


def test_fused_span_boundary():
    exact = np.arange(1000.0, 1000.0 + I.N_OUT)                              # speed exactly 1
    assert I.fused_usable_waves(exact, 379) == (14, 14)
    assert I.fused_usable_waves(exact, 380) == (1, 14)                       # (the partial last wave always fits)
    for name in ("c0.99", "c1.01", "sine"):
        st, sp, len_in = I.fused_curve(name, 0)
        pos, _ = C.speed_to_pos(st, sp, len_in)
        assert abs(len(pos) - I.N_OUT) < 60, (name, len(pos))
        usable, waves = I.fused_usable_waves(pos, 378)
        assert usable == waves, name
        assert I.fused_usable_waves(pos, 382)[0] <= 1, name
    st, sp, len_in = I.fused_curve("c0.3", 0)
    pos, _ = C.speed_to_pos(st, sp, len_in)
    assert abs(len(pos) - I.N_OUT) < 60
    assert I.fused_usable_waves(pos, 33)[0] >= 13 and I.fused_usable_waves(pos, 100)[0] <= 1


@pytest.mark.parametrize("NT", I.NT_SET)
def test_every_case_holds_the_lanes_it_is_named_for(NT):
    for regime, variant in I.CASES:
        pos, len_in, fc = I.positions(regime, variant, NT)
        assert np.all(np.diff(pos) > 0) and pos[0] > 0 and np.rint(pos[-1]) <= len_in - 1
        assert len_in <= 20000 and len(pos) <= I.N_OUT
        k = I.classify(pos, NT, len_in)
        what = (regime, variant, NT, k)
        if regime not in ("lead",):
            assert k["lead"] == 0, what
        if regime not in ("tail",):
            assert k["clipped"] == 0, what
        short = regime == "low" or (regime == "steep" and variant < 0.34)
        assert len(pos) == (360 if short else 2 * I.TILE + 328 if regime == "wide" else I.N_OUT)
        if not short and regime != "wide":
            assert k["staged"] == 4 and k["unstaged"] == 0 and k["low"] == 0, what
        if regime == "unity":
            assert k["fc_lt1"] == 0 and k["integer"] >= 2 * NT + 90 and k["half"] >= 99 and k["waves_unity"] == 16, what
            assert k["slow"] == 0, what
        elif regime == "gentle":
            assert k["fc1"] == 0 and k["groups_gentle"] == 28 and k["groups_steep"] == 0 and k["groups_edge"] == 0, what
            assert abs(np.median(I.periods(pos)) * fc - 1) < 1e-9
        elif regime == "gentle_edge":
            assert k["fc1"] == 0 and k["groups_gentle"] >= 4 and k["groups_steep"] >= 4, what
        elif regime == "steep":
            assert k["fc1"] == 0 and k["groups_steep"] == (4 if short else 28) and k["groups_gentle"] == 0, what
            assert k["slow"] == 0 and k["unstaged"] == 0 and k["low"] == 0, what
        elif regime == "mixed":
            assert k["fc1"] >= 1000 and k["fc_lt1"] >= 1000 and k["waves_mixed"] == 16 and k["waves_unity"] == 0, what
        elif regime == "low":
            assert k["staged"] == 1 and k["unstaged"] == 0, what
            if variant:
                assert k["low"] == k["n"] and k["fast"] == 0, what
            else:
                assert k["low"] == 0 and k["fast"] == k["n"] and k["groups_steep"] >= 1, what
                assert np.all(I.periods(pos) == 8.0)
        elif regime == "lead":
            assert NT - 2 <= k["lead"] <= NT + 40 and k["slow"] == k["lead"] and k["fast"] >= 1000, what
        elif regime == "tail":
            assert k["clipped"] >= NT - 1 and np.rint(pos[-1]) == len_in - 1, what
        elif regime == "wide":
            assert (k["staged"], k["unstaged"]) == ((1, 2) if variant else (3, 0)), what
            assert k["slow"] == (2 * I.TILE if variant else 0) and k["fc1"] == 0, what
    # both sides of the dd <= 0.5 branch of the seeding
    assert min(I.STEEP_FC) < 0.5 < max(I.STEEP_FC)


@pytest.mark.parametrize("NT", I.NT_SET)
def test_oracle_peaks_carry_the_bound(NT):
    for regime, variant in I.CASES:
        for name in I.SIGNALS:
            pos, sig = I.case_signal(name, regime, variant, NT)
            want = C.sinc(pos, sig, NT, threads=8)
            assert np.isfinite(want).all() and np.max(np.abs(want)) >= 0.1, (regime, variant, NT, name, float(np.max(np.abs(want))))


@pytest.mark.parametrize("NT", I.NT_NONFINITE)
def test_nonfinite_footprints(NT):
    for regime, variant in I.NONFINITE_CASES:
        pos, len_in, fc = I.positions(regime, variant, NT)
        mid = I.nonfinite_output(regime, NT, len(pos))
        period = float(np.median(I.periods(pos[max(mid - NT, 0):mid + NT])))
        for kind in ("nan", "inf"):
            sig, at = I.nonfinite_signal(kind, regime, variant, NT, pos, len_in)
            want = C.sinc(pos, sig, NT)
            bad = ~np.isfinite(want)
            assert np.array_equal(bad, I.footprint(pos, NT, len_in, at)), (regime, NT, kind)
            assert abs(int(bad.sum()) - 2 * NT / period) <= 2, (regime, NT, kind, int(bad.sum()), period)
            if regime == "unity":
                assert period == 1.0 and abs(int(bad.sum()) - 2 * NT) <= 2
            if kind == "nan":
                assert np.isnan(want[bad]).all()
            assert np.max(np.abs(want[~bad])) >= 0.1


@pytest.mark.parametrize("NT", [3, 101, 512])
def test_c_oracle_agrees_with_numpy_and_the_sum_is_well_conditioned(NT):
    for regime, variant in I.CASES:
        for name in I.SIGNALS:
            pos, sig = I.case_signal(name, regime, variant, NT)
            want = C.sinc(pos, sig, NT, threads=8)
            peak = float(np.max(np.abs(want)))
            every = 1 + NT // 64                                      # (a 2 NT-wide matrix per output: thinned out at the large NT)
            fwd, rev = I.sinc_f64(pos, sig, NT, every=every), I.sinc_f64(pos, sig, NT, reverse=True, every=every)
            assert np.max(np.abs(fwd - rev)) < 1e-7 * peak, (regime, variant, NT, name)
            assert np.max(np.abs(fwd - want[::every])) < 1.5e-7 * peak, (regime, variant, NT, name)       # float32 rounding of the output
            if name == "noise":
                assert np.max(np.abs(oracle_np.sinc_resample(pos, sig, NT) - want)) < 1.5e-7 * peak, (regime, variant, NT)
