"""GPU checks of the fixed-ratio resampler (K_rsfix, par_resample_fixed_f32, fixed_rate.resample), of the hum speed tool and of
the two opt-in resampling passes, against the float64 statement in tests/fixed_rate_np.py.

Every output is held to the derived bound (K[t] + 5) * 2^-24 * B[t] (fixed_rate_np.tolerance): the table entries, eta, the
weight and the products round once each in float32 and a float32 sum of K terms adds at most (K - 1) * 2^-24.  The worst
error / bound per case is printed (pytest -s)."""
import ctypes
import os

import numpy as np
import pytest

import fixed_rate_np as F

pytestmark = pytest.mark.gpu

SHAPES = [
    (48000, 44100, 700),                # step = 470, not a power of two
    (44100, 48000, 700),
    (44100, 44100 * 1.0417, 600),
    (44100, 44100 / 1.08, 600),
    (96000, 24000, 900),                # 63 taps
    (16, 1, 300),                       # 255 taps, the supported edge
    (1, 1, 40),
    (48000, 44100, 5),                  # shorter than one wing
]
SENTINEL = 0x7FC12345                   # a quiet NaN with a payload: compared as bits


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    return 0


def noise(n, seed, ch=None):
    return np.random.default_rng(seed).uniform(-1, 1, n if ch is None else (n, ch)).astype(np.float32)


def abi(dev, x_t, x_off, n, xs, a, b, y_t, y_off, n_out, ys, z=8):
    """par_resample_fixed_f32 on element offsets of two flat float32 device tensors"""
    from pyaudiorestoration_amd import _dev, _lib
    _lib.check(_lib.lib().par_resample_fixed_f32(dev, ctypes.c_void_p(x_t.data_ptr() + 4 * x_off), n, xs, float(a), float(b), z,
                                                 ctypes.c_void_p(y_t.data_ptr() + 4 * y_off), n_out, ys, _dev.stream_ptr(dev)))


def run(dev, x, a, b):
    import torch
    x_t = torch.from_numpy(np.ascontiguousarray(x)).to(f"cuda:{dev}")
    n_out = F.out_len(len(x), a, b)
    y_t = torch.empty(n_out, dtype=torch.float32, device=f"cuda:{dev}")
    abi(dev, x_t, 0, len(x), 1, a, b, y_t, 0, n_out, 1)
    return y_t.cpu().numpy()


def worst(got, y, K, B):
    tol = F.tolerance(K, B)
    err = np.abs(got.astype(np.float64) - y)
    assert np.all(err <= tol), (int(np.argmax(err - tol)), float(np.max(err - tol)))
    return float(np.max(err / np.where(tol > 0, tol, 1.0)))


@pytest.mark.parametrize("a,b,n", SHAPES, ids=[f"{a:g}-{b:g}-{n}" for a, b, n in SHAPES])
def test_every_output_within_the_derived_bound(dev, a, b, n):
    x = noise(n, 100 + n)
    y, K, B = F.oracle(x, a, b)
    got = run(dev, x, a, b)
    assert got.shape == y.shape and got.dtype == np.float32
    w = worst(got, y, K, B)
    print(f"fixed-ratio {a:g} -> {b:g}, n {n}: {len(y)} outputs, taps <= {K.max()}, worst error / bound {w:.3f}, bound <= {F.tolerance(K, B).max():.2e}")
    # the wings of the outputs at either end are cut by the signal's ends (the kernel's checked path); the middle is whole
    full = np.array([F.uncut_count(t, a, b) for t in range(len(K))])
    assert np.all(K <= full) and K[0] < full[0] and K[-1] < full[-1]
    assert np.any(K[:8] < full[:8]) and np.any(K[-8:] < full[-8:])
    if len(K) > 100:
        assert np.any(K == full)


def test_unit_impulse_returns_the_interpolated_weights(dev):
    x = np.zeros(64, dtype=np.float32)
    x[20] = 1.0
    y, K, B = F.oracle(x, 44100, 48000)
    got = run(dev, x, 44100, 48000)
    assert np.count_nonzero(y) >= 15
    worst(got, y, K, B)
    assert np.array_equal(got == 0, y == 0)                  # outputs whose taps miss the impulse are exact zeros


def test_positions_past_2_to_24(dev):
    """A float32 position is wrong from sample 2^24 on: the outputs around the one whose position crosses 2^24, and the last
    ones, against the oracle evaluated on those ranges only."""
    import torch
    n = (1 << 24) + 4099
    a, b = 44100, 48000
    x = noise(n, 7)
    n_out = F.out_len(n, a, b)
    x_t = torch.from_numpy(x).to(f"cuda:{dev}")
    y_t = torch.empty(n_out, dtype=torch.float32, device=f"cuda:{dev}")
    abi(dev, x_t, 0, n, 1, a, b, y_t, 0, n_out, 1)
    inc = 1.0 / (float(b) / a)
    t_cross = int(np.ceil((1 << 24) / inc))
    while t_cross * inc < (1 << 24):
        t_cross += 1
    assert (t_cross - 1) * inc < (1 << 24) <= t_cross * inc and t_cross + 1024 < n_out - 2048
    for t0, t1 in ((t_cross - 1024, t_cross + 1024), (n_out - 2048, n_out)):
        y, K, B = F.oracle(x, a, b, t0, t1)
        w = worst(y_t[t0:t1].cpu().numpy(), y, K, B)
        print(f"positions past 2^24: outputs [{t0}, {t1}) worst error / bound {w:.3f}")


@pytest.mark.parametrize("a,b", [(48000, 44100), (44100, 48000)], ids=["down", "up"])
def test_interleaved_channels_write_their_own_cells_only(dev, a, b):
    import torch
    n = 700
    x = noise(n, 11, ch=2)
    n_out = F.out_len(n, a, b)
    x_t = torch.from_numpy(x).to(f"cuda:{dev}").reshape(-1)
    for c in (0, 1):
        buf = torch.full(((n_out + 64) * 2,), SENTINEL, dtype=torch.int32, device=f"cuda:{dev}")
        y_t = buf.view(torch.float32)
        abi(dev, x_t, c, n, 2, a, b, y_t, c, n_out, 2)
        bits = buf.cpu().numpy().reshape(-1, 2)
        assert np.all(bits[:, 1 - c] == SENTINEL), "the other channel's cells were written"
        assert np.all(bits[n_out:, c] == SENTINEL), "cells past n_out were written"
        y, K, B = F.oracle(x[:, c], a, b)
        worst(bits[:n_out, c].copy().view(np.float32), y, K, B)


@pytest.mark.parametrize("a,b,n", [(48000, 44100, 5000), (44100, 48000, 5000), (16, 1, 3000)], ids=["down", "up", "sixteenth"])
def test_two_runs_are_bit_identical(dev, a, b, n):
    x = noise(n, 13)
    assert np.array_equal(run(dev, x, a, b).view(np.int32), run(dev, x, a, b).view(np.int32))


def test_wrapper_numpy_stereo_in_and_out(dev):
    import torch
    from pyaudiorestoration_amd import fixed_rate
    x = noise(700, 17, ch=2)
    for a, b in ((48000, 44100), (44100, 48000)):
        got = fixed_rate.resample(x, a, b, axis=0, filter="sinc_window", num_zeros=8)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (F.out_len(700, a, b), 2)
        for c in (0, 1):
            assert np.array_equal(got[:, c].view(np.int32), run(dev, x[:, c], a, b).view(np.int32))
        mono = fixed_rate.resample(x[:, 1], a, b)
        assert mono.shape == (len(got),) and np.array_equal(mono, got[:, 1])
        t = fixed_rate.resample(torch.from_numpy(x).to(f"cuda:{dev}"), a, b)
        assert torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and np.array_equal(t.cpu().numpy(), got)
    assert fixed_rate.resample(np.zeros((0, 2), dtype=np.float32), 48000, 44100).shape == (0, 2)
    z5 = fixed_rate.resample(x[:, 0], 44100, 48000, num_zeros=5)         # another table, the generic kernel at ratio >= 1
    y5, K5, B5 = F.oracle(x[:, 0], 44100, 48000, num_zeros=5)
    worst(z5, y5, K5, B5)


def test_renoiser_resamples_noise_at_another_rate_on_request(dev):
    """noise_profile(..., resample_noise=True) is noise_profile of the oracle-resampled noise, at the noise-profile tolerance of
    tests/test_renoiser_gpu.py (PROFILE_DB)."""
    from pyaudiorestoration_amd import renoiser
    from test_renoiser_gpu import PROFILE_DB
    noise_48k = noise(12000, 19)
    with pytest.raises(ValueError):
        renoiser.noise_profile(noise_48k, 48000, 44100)
    got = renoiser.noise_profile(noise_48k, 48000, 44100, resample_noise=True)
    y, _, _ = F.oracle(noise_48k, 48000, 44100)
    want = renoiser.noise_profile(y.astype(np.float32), 44100, 44100)
    err = float(np.max(np.abs(got - want)))
    print(f"renoiser profile of resampled noise: max |dB difference| {err:.2e}")
    assert got.shape == want.shape == (1025,) and err <= PROFILE_DB
    stereo = np.stack([noise_48k, -noise_48k[::-1]], axis=1)              # only the first channel is the profile
    assert np.array_equal(renoiser.noise_profile(stereo, 48000, 44100, resample_noise=True), got)


def mean_db_np(x, n_fft, hop):
    """np.mean(20 log10(|STFT| / sqrt(n_fft) + 1e-7), axis=frames) in float64: reflect padding, periodic float32 Hann window"""
    import scipy.signal
    x = np.asarray(x, dtype=np.float64)
    half = n_fft // 2
    p = np.pad(x, half, mode="reflect")
    nf = (len(x) + 2 * half - n_fft) // hop + 1
    w = scipy.signal.get_window("hann", n_fft).astype(np.float32).astype(np.float64)
    fr = p[np.arange(nf)[:, None] * hop + np.arange(n_fft)[None]] * w
    mag = np.abs(np.fft.rfft(fr, axis=1)) / np.sqrt(n_fft) + 1e-7
    return np.mean(20 * np.log10(mag), axis=0), nf


def test_get_spectrum_with_a_hop_longer_than_the_frame(dev, tmp_path):
    """hop = 2 * fft_size skips half the signal between frames: a new regime for the chunked mean.  Tolerance: the one
    tests/test_expander_gpu.py holds averaged spectra to (2e-2 dB within 60 dB of the peak)."""
    from pyaudiorestoration_amd import humspeed, io_ops
    x = noise(40000, 23, ch=2)
    path = str(tmp_path / "noise.wav")
    io_ops.write_wav_float(path, x, 44100)
    freqs, spectrum, sr = humspeed.get_spectrum(path, "L+R", fft_size=1024)
    m0, nf = mean_db_np(x[:, 0], 1024, 2048)
    m1, _ = mean_db_np(x[:, 1], 1024, 2048)
    want = np.mean([m0, m1], axis=0)
    assert nf == 20 and sr == 44100 and spectrum.shape == want.shape == freqs.shape == (513,)
    assert freqs[1] == 44100 / 1024
    top = want >= want.max() - 60
    err = float(np.max(np.abs(spectrum - want)[top]))
    print(f"get_spectrum fft 1024 hop 2048: max |dB difference| {err:.2e} over {top.mean():.0%} of the bins")
    assert top.mean() > 0.9 and err <= 2e-2
    left = humspeed.get_spectrum(path, "L", fft_size=1024)[1]
    assert float(np.max(np.abs(left - m0)[top])) <= 2e-2


def test_analyse_finds_a_detuned_hum_at_the_full_size(dev, tmp_path):
    """3 * 2^19 samples of a 50.7 Hz tone (a cosine, so the reflected first frame continues it) plus noise, the GUI's 2^19-point
    frames: the ratio is 50 / 50.7 within 1e-4."""
    from pyaudiorestoration_amd import humspeed, io_ops
    n, sr = 3 << 19, 44100
    x = (0.5 * np.cos(2 * np.pi * 50.7 * np.arange(n) / sr) + 0.01 * noise(n, 29)).astype(np.float32)
    path = str(tmp_path / "hum.wav")
    io_ops.write_wav_float(path, x, sr)
    res = humspeed.analyse(path, num_harmonies=0)
    assert res["spectrum"].shape == (262145,) and res["sr"] == sr and list(res["hum_freqs"]) == [50]
    assert len(res["ratios"]) == 1 and len(res["marker_freqs"]) == 1 and len(res["marker_dBs"]) == 1
    print(f"analyse: hum at {res['marker_freqs'][0]:.5f} Hz, ratio {res['ratios'][0]:.7f} (50 / 50.7 = {50 / 50.7:.7f})")
    assert abs(res["ratios"][0] - 50 / 50.7) <= 1e-4


def test_resample_file_round_trip(dev, tmp_path):
    from pyaudiorestoration_amd import fixed_rate, humspeed, io_ops
    n, sr, ratio = 4999, 44100, 50 / 50.7
    x = noise(n, 31, ch=2)
    path = str(tmp_path / "tape.wav")
    io_ops.write_wav_float(path, x, sr)
    out = humspeed.resample_file(path, ratio)
    assert out == str(tmp_path / "tape_resampled_-1.381.wav") and os.path.exists(out)
    y, sr_out, ch = io_ops.read_file(out)
    assert sr_out == sr and ch == 2 and y.shape == (int(n / ratio), 2) == (5068, 2)
    assert np.array_equal(y, fixed_rate.resample(x, sr * ratio, sr))
    y0, K, B = F.oracle(x[:, 0], sr * ratio, sr)
    worst(y[:, 0], y0, K, B)


def test_correlate_sources_match_speed_resamples_the_source(dev):
    """match_speed=True is the caller-side resampling of the reference's match_speed branch, done inside."""
    from pyaudiorestoration_amd import fixed_rate, pipeline
    sr, speed = 44100, 1.03
    ref = noise(20000, 37)
    src = noise(int(20000 / speed), 41)
    d1, c1 = pipeline.correlate_sources(ref, src, sr, 100, 2000, speed=speed, match_speed=True)
    d2, c2 = pipeline.correlate_sources(ref, fixed_rate.resample(src, sr / speed, sr), sr, 100, 2000, speed=speed)
    assert d1 == d2 and c1 == c2
