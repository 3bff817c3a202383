"""CPU side of the group-delay feature: the band edges, the float64 statement of the flow against the reference's recorded run
(tests/golden/group_delay.npz, tools/gen_golden_group_delay.py), the numpy model of par_find_delay_sect_f64's diagonal scheme, and
the entry point's argument checks, which come before any device call."""
import ctypes
import functools
import os

import numpy as np
import pytest

import group_delay_np as G
import xcorr_inputs as X


@functools.lru_cache(maxsize=None)
def model_bands():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "group_delay.npz"))
    return g, G.measure_np(g["ref"], g["src"], int(g["sr"]), g["band_limits"])


def test_band_limits_are_the_references_truncated_logspace():
    from pyaudiorestoration_amd import group_delay
    g, _ = model_bands()
    edges = group_delay.band_limits()
    assert edges.dtype == np.uint16 and np.array_equal(edges, g["band_limits"]) and edges[0] == 9 and len(edges) == 44
    assert np.array_equal(group_delay.band_limits(10, 2000, 45), edges)
    with pytest.raises(ValueError, match="band 1 .* 10 Hz"):
        group_delay.band_limits(10, 2000, 10)                # 199 edges: 9 (10 rounded down in base 2), then 10.27 and 10.55 -> 10, 10


def test_fixture_preconditions():
    """most bands kept, one rejected (the test of the threshold), and no kept peak near either end of the 'same' span"""
    g, bands = model_bands()
    kept = [b for b in bands if b.corr > G.MIN_CORR]
    assert len(bands) == 43 and len(kept) >= 35 and len(kept) < len(bands)
    assert all(b.status == 0 and b.oracle is not None for b in bands)
    na = len(g["ref"])
    assert all(3 <= b.oracle.peak <= na - 4 for b in kept)
    assert np.array_equal(G.fixture_signals()[0], g["ref"]) and np.array_equal(G.fixture_signals()[1], g["src"])


def test_host_statement_reproduces_the_references_run():
    """the kept set exactly; lags and correlations within flow_bounds' formula (windows of ones; the filter's share is zero here,
    both sides filter with scipy); centres exactly; level differences to the rounding of two norms"""
    g, bands = model_bands()
    kept = [b for b in bands if b.corr > G.MIN_CORR]
    centers = np.array([(float(b.lo) + float(b.hi)) / 2 for b in kept])
    assert np.array_equal(centers, g["band_centers"])
    worst = [0.0, 0.0]
    for b, lag, corr, mag in zip(kept, g["lags"], g["correlations"], g["magnitudes"]):
        bd, bc = G.bounds(b.oracle, len(b.yb))
        worst = [max(worst[0], abs(b.lag - lag) / bd), max(worst[1], abs(b.corr - corr) / bc)]
        assert abs(b.lag - lag) <= bd and abs(b.corr - corr) <= bc, (b.lo, b.hi, b.lag - lag, bd, b.corr - corr, bc)
        assert abs((b.level_ref - b.level_src) - mag) <= 4 * X.U * (b.level_ref + b.level_src)
    print(f"worst share of the bound: lag {worst[0]:.3f}, corr {worst[1]:.3f}")


S = 4096
DIAG_SHAPES = ((3 * S + 5, 2 * S - 1), (S + 1, S + 1), (4 * S, 4 * S), (3000, 3000))


@pytest.mark.parametrize("na,nb", DIAG_SHAPES)
def test_diagonal_model_equals_the_full_correlation(na, nb):
    rng = np.random.default_rng([91, na, nb])
    a, b = rng.standard_normal(na), 0.5 * rng.standard_normal(nb)
    b[:min(na, nb) - 40] += a[40:min(na, nb)]
    want = X.full_fft(a, b)
    got, count = G.diag_full(a, b, S)
    assert got.shape == want.shape and np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
    assert count.max() <= 2 and count.min() >= 1
    P, Q = -(-na // S), -(-nb // S)
    lags = np.arange(-(nb - 1), na)
    d0 = lags // S
    want_count = ((d0 >= -(Q - 1)) & (d0 <= P - 1)).astype(int) + ((lags % S > 0) & (d0 + 1 >= -(Q - 1)) & (d0 + 1 <= P - 1))
    assert np.array_equal(count, want_count)              # the two terms the Lags functor of the kernels adds: d0 = floor(l / S), d0 + 1


def test_sectioned_entry_checks_its_arguments_before_any_device_call():
    from pyaudiorestoration_amd import _lib
    L = _lib.lib()
    one = L.par_find_delay_sect_scratch_bytes(3000, 3000, 1, 12)
    tables = one - 2 * 1 * 8192 * 8                       # the row record: the size is the library's, not assumed
    assert 0 < tables < 4096
    # all rows in one pass: P = 4, Q = 2 -> D = 5 arrays of N = 8192 points, twice, per row
    assert L.par_find_delay_sect_scratch_bytes(3 * S + 5, 2 * S - 1, 3, 12) == 3 * (2 * 5 * 8192 * 8 + tables)
    assert L.par_find_delay_sect_scratch_bytes(3000, 3000, 0, 12) == one
    assert L.par_find_delay_sect_scratch_bytes(3000, 3000, 1, 0) == 2 * (1 << 20) * 8 + tables          # 0 means 2^19
    assert L.par_find_delay_sect_scratch_bytes(1 << 25, 1 << 25, 5, 0) == 2 * 127 * (1 << 20) * 8 + tables  # never less than one row
    capped = L.par_find_delay_sect_scratch_bytes(3000, 3000, 100000, 12)
    assert capped == 8192 * one                           # 1 GiB of transform arrays
    for bad in ((0, 5, 1, 12), (5, 0, 1, 12), ((1 << 25) + 1, 5, 1, 12), (5, 5, 1, 11), (5, 5, 1, 20), (5, 5, 1, -1)):
        assert L.par_find_delay_sect_scratch_bytes(*bad) == 0, bad
    p = ctypes.c_void_p(8)
    good = dict(a=p, a_pitch=3000, na=3000, b=p, b_pitch=3000, nb=3000, n_win=2, sec=12, scratch=p, nbytes=2 * one, delay=p, corr=p,
                status=p, norms=None, same=None, same_pitch=0)

    def call(**change):
        k = dict(good, **change)
        return L.par_find_delay_sect_f64(0, k["a"], k["a_pitch"], k["na"], k["b"], k["b_pitch"], k["nb"], k["n_win"], k["sec"], 0,
                                         k["scratch"], k["nbytes"], k["delay"], k["corr"], k["status"], k["norms"], k["same"],
                                         k["same_pitch"], None)
    for name in ("a", "b", "scratch", "delay", "corr", "status"):
        assert call(**{name: None}) == 1 and "null pointer" in _lib.last_error(), name
    for change, text in ((dict(na=2), "na 2"), (dict(nb=0), "nb 0"), (dict(n_win=-1), "n_win -1"), (dict(a_pitch=2999), "pitch 2999"),
                         (dict(b_pitch=2999), "pitch 3000 / 2999"), (dict(same=p, same_pitch=2999), "pitch 3000 / 3000 / 2999"),
                         (dict(sec=11), "section_log2 11"), (dict(sec=20), "section_log2 20"), (dict(sec=-1), "section_log2 -1")):
        assert call(**change) == 1 and text in _lib.last_error(), (change, _lib.last_error())
    assert call(n_win=0) == 0 and call(n_win=0, nbytes=0) == 0
    assert call(na=(1 << 25) + 1, a_pitch=1 << 26) == 3 and "2^25" in _lib.last_error()
    assert call(nb=(1 << 25) + 1, b_pitch=1 << 26) == 3
    assert call(nbytes=one - 1) == 4 and "less than one row" in _lib.last_error()
    assert call(nbytes=0) == 4
    with pytest.raises(_lib.ParUnsupported):
        _lib.check(call(na=(1 << 25) + 1, a_pitch=1 << 26))


def test_filter_phase_delay_is_the_scripts_arithmetic():
    """experiments/group_delay.py:124-138 for one filter: freqz_sos, unwrap, -phase / (2 pi) * sr / f"""
    import scipy.signal
    from pyaudiorestoration_amd import group_delay
    sr = 44100
    sos = scipy.signal.bessel(1, 50, "low", analog=False, output="sos", fs=sr)
    f, delay = group_delay.filter_phase_delay(sos, sr)
    w, h = scipy.signal.sosfreqz(sos)
    phase = np.unwrap(np.angle(h))
    want_f = w / np.pi * sr / 2
    with np.errstate(all="ignore"):
        want = -(phase / (2 * np.pi)) * sr / want_f
    assert len(f) == 512 and np.array_equal(f, want_f) and np.array_equal(delay[1:], want[1:]) and not np.isfinite(delay[0])
    analog = np.arctan(f[1:20] / 50) / (2 * np.pi * f[1:20]) * sr            # the phase delay of the analog first-order low-pass, in samples
    assert np.all(np.abs(delay[1:20] - analog) < 0.02 * analog)
