"""CPU-only checks of the fixed-ratio resampler's host side (par_resample_fixed_out_len, the argument checks of
par_resample_fixed_f32), of the float64 oracle the GPU tests hold the kernel against (tests/fixed_rate_np.py), and of the hum
speed tool's host arithmetic against the reference's own results (tests/golden/humspeed.npz, tools/gen_golden_humspeed.py)."""
import ctypes

import numpy as np
import pytest

import fixed_rate_np as F


def test_out_len_is_pythons_left_to_right_product():
    from pyaudiorestoration_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(20240)
    rates = [8000.0, 11025.0, 22050.0, 44100.0, 48000.0, 88200.0, 96000.0, 192000.0, 44100 * 1.0417, 44100 / 1.08, 50 / 50.7 * 48000]
    differ = 0
    for _ in range(4000):
        n = int(rng.integers(0, 700_000_000))
        a, b = float(rng.choice(rates)), float(rng.choice(rates))
        want = int(n * b / a)
        assert L.par_resample_fixed_out_len(n, a, b) == want, (n, a, b)
        differ += want != int(n * (b / a))
    assert differ > 0, "the sweep must hold cases where int(n * (sr_new / sr_orig)) is another number"
    assert L.par_resample_fixed_out_len(700, 48000.0, 44100.0) == 643 and L.par_resample_fixed_out_len(700, 44100.0, 48000.0) == 761
    for bad in ((-1, 1.0, 1.0), (5, 0.0, 1.0), (5, 1.0, -2.0), (5, float("nan"), 1.0), (5, 1.0, float("inf"))):
        assert L.par_resample_fixed_out_len(*bad) == -1


def test_argument_errors_touch_no_device():
    from pyaudiorestoration_amd import _lib
    L = _lib.lib()
    p, q = ctypes.c_void_p(64), ctypes.c_void_p(4096)
    n, a, b = 700, 48000.0, 44100.0
    m = L.par_resample_fixed_out_len(n, a, b)

    def call(dev=0, x=p, n_=n, xs=1, a_=a, b_=b, z=8, y=q, m_=m, ys=1):
        return L.par_resample_fixed_f32(dev, x, n_, xs, a_, b_, z, y, m_, ys, None)
    assert call(x=None) == 1 and "null" in _lib.last_error()
    assert call(y=None) == 1
    for rate in (0.0, -44100.0, float("nan"), float("inf")):
        assert call(a_=rate) == 1 and "rates" in _lib.last_error()
        assert call(b_=rate) == 1
    assert call(z=0) == 1 and "num_zeros" in _lib.last_error()
    assert call(z=65) == 1
    assert call(m_=m + 1) == 1 and "n_out" in _lib.last_error()
    assert call(m_=int(n * (b / a)) + 1) == 1
    assert call(xs=0) == 1 and "stride" in _lib.last_error()
    assert call(ys=0) == 1 and call(ys=-2) == 1
    assert call(y=p) == 1 and "same buffer" in _lib.last_error()
    assert call(n_=-1, m_=0) == 1
    # nothing to do: PAR_OK without a device call (no GPU here, and device 99 exists nowhere)
    assert call(dev=99, n_=0, m_=0) == 0
    assert call(dev=99, n_=3, a_=48000.0, b_=8000.0, m_=0) == 0
    # outside [1/16, 16]: unsupported, named before any device call
    assert call(dev=99, a_=17.0, b_=1.0, m_=L.par_resample_fixed_out_len(n, 17.0, 1.0)) == 3 and "ratio" in _lib.last_error()
    assert call(dev=99, a_=1.0, b_=16.5, m_=L.par_resample_fixed_out_len(n, 1.0, 16.5)) == 3
    with pytest.raises(_lib.ParUnsupported):
        _lib.check(3)


def test_wrapper_refuses_what_it_does_not_do():
    from pyaudiorestoration_amd import fixed_rate
    x = np.zeros((10, 2), dtype=np.float32)
    with pytest.raises(ValueError, match="axis"):
        fixed_rate.resample(x, 48000, 44100, axis=1)
    with pytest.raises(ValueError, match="sinc_window"):
        fixed_rate.resample(x, 48000, 44100, filter="kaiser_best")
    with pytest.raises(ValueError, match="num_zeros"):
        fixed_rate.resample(x, 48000, 44100, num_zeros=0)
    with pytest.raises(ValueError, match="rates"):
        fixed_rate.resample(x, 0, 44100)
    assert fixed_rate.out_len(700, 48000, 44100) == 643 and fixed_rate.out_len(700, 44100, 48000) == 761


def test_oracle_on_a_unit_impulse_returns_the_table():
    """x = delta at sample 20: output t sees it through exactly one tap, whose weight is the interpolated table look-up."""
    win, delta = F.table(8)
    assert len(win) == 4097 and win[0] == F.ROLLOFF and abs(win[-1]) < 1e-18 and delta[-1] == 0.0
    x = np.zeros(64)
    x[20] = 1.0
    y, K, B = F.oracle(x, 44100, 48000)
    assert len(y) == F.out_len(64, 44100, 48000) == 69
    seen = 0
    for t in range(len(y)):
        jl, il, el, jr, ir, er, scale = F.taps(t, 64, 44100, 48000)
        want = 0.0
        for j, i, e in ((jl, il, el), (jr, ir, er)):
            hit = np.nonzero(i == 20)[0]
            assert len(hit) <= 1
            if len(hit):
                want += win[j[hit[0]]] + e * delta[j[hit[0]]]
                seen += 1
        assert y[t] == want
        assert K[t] == len(jl) + len(jr) <= 16
    assert seen >= 15 and 0.8 < np.max(np.abs(y)) <= F.ROLLOFF   # the main lobe (peak = rolloff) passes over the impulse


def test_oracle_at_ratio_one_uses_offsets_0_and_512_only():
    x = np.random.default_rng(3).uniform(-1, 1, 40)
    for t in range(40):
        jl, il, el, jr, ir, er, scale = F.taps(t, 40, 1, 1)
        assert scale == 1.0 and el == 0.0 and er == 0.0
        assert set(jl % 512) == {0} and set(jr % 512) <= {0} and jl[0] == 0 and (len(jr) == 0 or jr[0] == 512)
        assert il[0] == t
    y, K, B = F.oracle(x, 1, 1)
    win, _ = F.table(8)
    # the taps at the zero crossings are not exactly zero (rolloff 0.945 moves them off the crossings): it is a filter, not a copy
    full = slice(8, 32)
    assert np.all(K[full] == 8 + 7) and np.all(K[:7] < 15) and np.all(K[-7:] < 15)
    assert abs(y[20] - sum(win[512 * i] * x[20 - i] for i in range(8)) - sum(win[512 * (k + 1)] * x[21 + k] for k in range(7))) < 1e-15


def test_tap_counts_at_the_supported_edges():
    assert max(F.oracle(np.ones(300), 16, 1)[1]) == 255
    assert max(F.oracle(np.ones(900), 96000, 24000)[1]) == 63           # 32 + 31: both wings hold 32 only at offsets <= 1
    assert max(F.oracle(np.ones(900), 96000, 24001)[1]) <= 64
    assert max(F.oracle(np.ones(700), 44100, 48000)[1]) <= 16
    y, K, B = F.oracle(np.ones(700), 48000, 44100)
    full = np.array([F.uncut_count(t, 48000, 44100) for t in range(len(K))])
    assert np.all(K <= full) and K[0] < full[0] and K[-1] < full[-1] and np.array_equal(K[20:-20], full[20:-20])


def test_oracle_against_installed_resampy():
    resampy = pytest.importorskip("resampy")
    rng = np.random.default_rng(5)
    for n, a, b in ((700, 48000, 44100), (700, 44100, 48000), (900, 96000, 24000)):
        x = rng.uniform(-1, 1, n)
        want = resampy.resample(x, a, b, axis=0, filter="sinc_window", num_zeros=8)
        y, _, _ = F.oracle(x, a, b)
        assert y.shape == want.shape and np.max(np.abs(y - want)) <= 1e-12


# ------------------------------------------------------------------------------------------------ hum speed tool (host arithmetic)
def test_hum_freqs_and_track_to_against_the_reference(golden):
    from pyaudiorestoration_amd import fourier, humspeed
    g = golden["humspeed"]
    fft = int(g["fft_size"])
    assert sorted(g["cases"]) == ["coarse", "first_bin", "harmonics2", "harmonics3", "inside", "rejected"]
    for name in g["cases"]:
        sr, tol, xpos, base, harm = g[f"{name}_params"]
        spectrum = g[f"{name}_spectrum"]
        assert spectrum.shape == (2049,)
        freqs = fourier.fft_freqs(fft, sr)
        hums = humspeed.hum_freqs(int(base), int(harm))
        assert np.array_equal(hums, g[f"{name}_hum_freqs"]) and hums.dtype == g[f"{name}_hum_freqs"].dtype
        targets = hums if xpos < 0 else [xpos]
        found = [humspeed.track_to(freqs, spectrum, sr, fft, x, hums, tol) for x in targets]
        kept = [f for f in found if f is not None]
        assert np.array_equal([f[0] for f in kept], g[f"{name}_marker_freqs"]), name
        assert np.array_equal([f[1] for f in kept], g[f"{name}_marker_dBs"]), name
        assert np.array_equal([f[2] for f in kept], g[f"{name}_ratios"]), name
        texts = list(g[f"{name}_texts"])
        assert [f is None for f in found] == [t == "hum was not close enough" for t in texts], name
        for f, t in zip(found, texts):
            if f is not None:
                assert t == "Percent Change: " + "%.3f" % ((f[2] - 1) * 100)
    assert len(g["rejected_ratios"]) == 0 and len(g["harmonics3_ratios"]) == 4 and len(g["harmonics2_ratios"]) == 2
    assert g["first_bin_marker_freqs"][0] < 46.5                       # the raw peak is the band's first bin (46 Hz)
    assert humspeed.resampled_suffix(50 / 50.7) == "_resampled_-1.381"


def test_cli_parser_knows_humspeed_and_resample_noise():
    from pyaudiorestoration_amd import cli
    a = cli.parser().parse_args(["humspeed", "a.wav", "b.flac"])
    assert (a.cmd, a.channels, a.hum, a.harmonies, a.tolerance, a.fft, a.resample, a.files) == \
        ("humspeed", "L+R", 50, 2, 8, 524288, False, ["a.wav", "b.flac"])
    a = cli.parser().parse_args(["humspeed", "--channels", "L", "--hum", "60", "--harmonies", "3", "--tolerance", "4", "--fft", "262144",
                                 "--resample", "a.wav"])
    assert (a.channels, a.hum, a.harmonies, a.tolerance, a.fft, a.resample) == ("L", 60, 3, 4, 262144, True)
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["humspeed", "--channels", "Mean", "a.wav"])
    assert cli.parser().parse_args(["renoise", "--noise", "h.wav", "a.wav"]).resample_noise is False
    assert cli.parser().parse_args(["renoise", "--noise", "h.wav", "--resample-noise", "a.wav"]).resample_noise is True


def test_renoiser_still_refuses_another_rate_by_default():
    import inspect
    from pyaudiorestoration_amd import pipeline, renoiser
    with pytest.raises(ValueError, match="sample rate"):
        renoiser.noise_profile(np.zeros(4096, dtype=np.float32), 48000, 44100)
    with pytest.raises(ValueError, match="sample rate"):
        renoiser.noise_profile(np.zeros(4096, dtype=np.float32), 48000, 44100, resample_noise=False)
    assert inspect.signature(renoiser.noise_profile).parameters["resample_noise"].default is False
    assert inspect.signature(renoiser.renoise_file).parameters["resample_noise"].default is False
    assert inspect.signature(pipeline.correlate_sources).parameters["match_speed"].default is False
