"""Host side of the zero-crossing flutter analysis (pyaudiorestoration_amd/zerocrossing_wow.py) and its yardsticks
(tests/zerocross_np.py), without a GPU.  The bounds and their derivations are in zerocross_np's docstring."""
import collections

import numpy as np
import pytest

import zerocross_np as Z

KEYS = ("a", "b")


@pytest.mark.parametrize("n", range(2, 10))
def test_fold_is_numpys_reflect_pad_at_every_width(n):
    """k = q mod 2 (n - 1), k >= n -> 2 (n - 1) - k against np.pad(mode="reflect"), widths 1 .. 3 n: single, exact and repeated
    reflection"""
    a = np.arange(n)
    for width in range(1, 3 * n + 1):
        assert np.array_equal(Z.reflect_index(n, width), np.pad(a, width, mode="reflect")), (n, width)


@pytest.mark.parametrize("n,span", [(2, 1), (2, 2), (3, 3), (5, 4), (5, 5), (5, 9), (9, 7), (9, 8), (40, 17), (100, 80)])
def test_fraction_sum_and_numpys_convolution_agree_under_the_bound(n, span):
    """exact_smooth (Fractions, one rounding) against np.pad + np.convolve(mode="same")[span:-span]: numpy's sum is a float64 sum
    of span non-negative rounded products in some order, so it lies within (span + 2) 2^-53 of the exact value (zerocross_np).
    Also pins the centring (span - 1) // 2 for both parities."""
    rng = np.random.default_rng(n * 100 + span)
    d = rng.integers(1, 41, n).astype(np.float32)
    kernel = Z.hann_kernel(span)
    exact, got = Z.exact_smooth(d, kernel), Z.numpy_smooth(d, kernel)
    assert got.shape == exact.shape == (n,)
    assert np.all(np.abs(got - exact) <= Z.bound_smooth(span) * exact)
    if span == 1:
        assert np.array_equal(exact, 2.0 * d)              # the reference's quirk at span 1: the one weight is 2


@pytest.mark.parametrize("key", KEYS)
def test_smoothing_span_is_the_reference_size_on_the_golden_pilots(golden, key):
    """(last - first) / n in float64 against the reference's float32 np.mean: the same `size` wherever the quotient is not within
    about 2^-20 of an integer; the fixtures keep 1e-3 away (asserted when they were made, and here)"""
    from pyaudiorestoration_amd import zerocrossing_wow as zc
    g = golden["zerocrossing"]
    c = g[f"{key}_crossings"]
    q = float(g[f"{key}_quotient"])
    assert abs(q - round(q)) >= 1e-3
    assert zc.smoothing_span(int(g[f"{key}_sr"]), c[0], c[-1], len(c) - 1) == int(g[f"{key}_size"]) == int(q)
    # the reference's own expression on the same crossings
    assert int(int(g[f"{key}_sr"]) / 100 / np.mean(Z.periods(c))) == int(g[f"{key}_size"])
    assert abs(float(np.mean(Z.periods(c))) - float(g[f"{key}_mean"])) <= 1e-6 * float(g[f"{key}_mean"])     # as printed


def test_smoothing_span_below_one_is_a_value_error():
    """a pilot under 50 Hz: the reference's np.convolve raises ValueError("v cannot be empty")"""
    from pyaudiorestoration_amd import zerocrossing_wow as zc
    assert zc.smoothing_span(48000, 0, 4800, 10) == 1           # exactly 50 Hz
    with pytest.raises(ValueError, match="v cannot be empty"):
        zc.smoothing_span(48000, 0, 4810, 10)
    with pytest.raises(ValueError):
        np.convolve(np.ones(5), np.ones(0), mode="same")


@pytest.mark.parametrize("key", KEYS)
def test_golden_curves_are_consistent_with_the_yardsticks(golden, key):
    """The stored curves of the reference's run against zerocross_np on the stored crossings: times and the float32 raw curve
    bit for bit; the smoothed curve against numpy_chain (the same statement: bit for bit as long as numpy's convolution keeps its
    order, and always under 2 (span + 4) 2^-53) and against the exact sum under (span + 4) 2^-53 for the division's result."""
    g = golden["zerocrossing"]
    sr, c, span = int(g[f"{key}_sr"]), g[f"{key}_crossings"], int(g[f"{key}_size"])
    x = (g[f"{key}_signal"] / 32768.0).astype(np.float32)
    pos = x > 0
    assert np.array_equal(np.where(pos[1:] != pos[:-1])[0], c)
    ch = Z.numpy_chain(c, sr, span)
    assert np.array_equal(ch["xp"], g[f"{key}_raw_t"]) and np.array_equal(ch["xp"], g[f"{key}_t"])
    assert g[f"{key}_raw_f"].dtype == np.float32 and np.array_equal(ch["raw"], g[f"{key}_raw_f"])
    f = g[f"{key}_f"]
    assert f.dtype == np.float64 and np.all(np.abs(ch["freq"] - f) <= Z.bound_vs_numpy(span) * f)
    exact = (sr / 2) / Z.exact_smooth(ch["d"], Z.hann_kernel(span))
    assert np.all(np.abs(f - exact) <= Z.bound_freq(span) * exact)


Result = collections.namedtuple("Result", "raw_times raw_freqs times freqs span grid_times grid_freqs")


def test_speed_curve_and_report_on_a_hand_made_result():
    from pyaudiorestoration_amd import pipeline, zerocrossing_wow as zc
    t = np.arange(5) * 0.01
    f = np.array([1000.0, 1010.0, 1000.0, 990.0, 1000.0])
    res = Result(t, f.astype(np.float32), t, f, 7, t, f)
    curve = zc.speed_curve(res)
    assert curve.shape == (5, 2) and curve.dtype == np.float64 and np.array_equal(curve[:, 0], t)
    assert np.array_equal(curve[:, 1], 2.0 ** pipeline.trace_to_speed(f))
    assert abs(np.prod(curve[:, 1]) - 1.0) < 1e-12                      # log2 speed is centred on 0
    rep = zc.report(res)
    assert rep["span"] == 7 and rep["crossings"] == 6 and rep["mean_hz"] == 1000.0
    assert abs(rep["peak_to_peak_percent"] - 2.0) < 1e-12 and abs(rep["rms_percent"] - np.sqrt(0.4)) < 1e-12
    with pytest.raises(ValueError, match="hop"):
        zc.speed_curve(Result(t, f, t, f, 7, None, None))
    assert zc.report(Result(t, f, t, f, 7, None, None))["mean_hz"] == 1000.0      # without a grid: the per-crossing curve
    assert np.array_equal(zc.grid(1000, 48000, 256), np.arange(4) * (256 / 48000))
    assert np.array_equal(zc.hann_kernel(80), Z.hann_kernel(80))


def test_fewer_than_three_crossings_is_a_value_error():
    """before any device is asked for: it raises on a machine without one"""
    import torch
    from pyaudiorestoration_amd import zerocrossing_wow as zc
    for c in (0, 1, 2):
        with pytest.raises(ValueError, match="at least 3"):
            zc.smooth_crossings_dev(torch.arange(c, dtype=torch.int64) * 10, 48000)


def test_flutter_cli_arguments():
    from pyaudiorestoration_amd import cli
    a = cli.parser().parse_args(["flutter", "tape.flac"])
    assert (a.cmd, a.files, a.band, a.hop, a.channel, a.json, a.resample, a.order) == ("flutter", ["tape.flac"], None, 256, "L", None,
                                                                                       False, 3)
    a = cli.parser().parse_args(["flutter", "--band", "3000,5000", "--hop", "64", "--channel", "R", "--json", "r.json", "--resample",
                                 "a.wav", "b.wav"])
    assert (a.band, a.hop, a.channel, a.json, a.resample, a.files) == ([3000.0, 5000.0], 64, "R", "r.json", True, ["a.wav", "b.wav"])
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["flutter", "--channel", "M", "tape.flac"])
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["flutter"])


def test_argument_errors_of_the_entry_points_come_before_any_device_call():
    """PAR_ERR_ARG (1) with the reason named; no GPU is needed to be refused"""
    import ctypes
    from pyaudiorestoration_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(8)
    good = dict(crossings=p, c=10, kernel=p, span=3, sr=48000.0, t0=0.0, smooth=None, freq=p, xp=p, raw=None)

    def smooth(**kw):
        a = dict(good, **kw)
        return L.par_crossing_smooth_f64(0, a["crossings"], a["c"], a["kernel"], a["span"], a["sr"], a["t0"], a["smooth"], a["freq"],
                                         a["xp"], a["raw"], None)
    for change, text in [(dict(crossings=None), "null"), (dict(kernel=None), "null"), (dict(freq=None), "null"), (dict(xp=None), "null"),
                         (dict(c=2), "at least 3"), (dict(span=0), "span 0"), (dict(span=_lib.CROSSING_SMOOTH_MAX_SPAN + 1), "span"),
                         (dict(sr=0.0), "sample rate"), (dict(sr=-1.0), "sample rate"), (dict(sr=float("nan")), "sample rate"),
                         (dict(sr=float("inf")), "sample rate")]:
        assert smooth(**change) == 1 and text in _lib.last_error(), change
    assert _lib.CROSSING_SMOOTH_MAX_SPAN >= 4096
    assert L.par_interp_f64(0, None, 0, p, p, 1, None, None) == 0                  # nx == 0: nothing to do
    for args, text in [((p, 4, None, p, 2, p), "null"), ((p, 4, p, None, 2, p), "null"), ((None, 4, p, p, 2, p), "null"),
                       ((p, 4, p, p, 2, None), "null"), ((p, 4, p, p, 0, p), "m >= 1"), ((p, -1, p, p, 2, p), "nx >= 0")]:
        assert L.par_interp_f64(0, *args, None) == 1 and text in _lib.last_error(), args
