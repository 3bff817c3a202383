"""Cyclic wow without a GPU: the numpy restatement (tests/cyclic_np.py) against the reference's own results in
tests/golden/cyclic.npz, the preconditions of that fixture, the host parts of pyaudiorestoration_amd.cyclic_wow, and the argument
errors of par_stft_track_peak_f64 / par_cycle_fold_f64, all of which return before any device call."""
import ctypes
import os

import numpy as np
import pytest

import cyclic_np as C
from pyaudiorestoration_amd import cyclic_wow as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PILOT = os.path.join(ROOT, "tests", "golden", "cyclic_pilot.wav")


@pytest.fixture(scope="module")
def g(golden):
    return {k: v for k, v in golden["cyclic"].items()}


@pytest.fixture(scope="module")
def pilot_db(g):
    """the float64 spectrogram the reference's numpy backend gave its script, in dB: [frames][bins] float64 and rounded to float32"""
    from oracle import oracle_np as O
    from pyaudiorestoration_amd import io_ops
    x, sr, ch = io_ops.read_file(PILOT)
    assert (sr, ch, len(x)) == (int(g["sr"]), 1, 264600)
    mag = np.ascontiguousarray(O.get_mag(x[:, 0], int(g["fft_size"]), int(g["hop"]), "hann", 1).T)
    return 20 * np.log10(mag), C.to_db32(mag)


def test_fold_and_search_equal_the_reference_bit_for_bit(g):
    """np.mean over the views adds view after view: the ordered restatement, np.mean itself and the reference agree to the bit"""
    lf = np.log2(g["freqs"])
    init, tol = int(g["frames_per_rotation_init"]), float(g["tolerance"])
    assert (init, int(g["d"])) == (229, 22) and init == int(60.0 / float(g["rpm"]) * int(g["sr"]) / int(g["hop"]))
    assert W.candidate_range(init, tol) == (207, 44, 22)
    results = C.search(lf, init, tol)
    assert results.shape == (44, 2) and np.array_equal(results, g["results"])
    best = results[np.argmax(results[:, 1])]
    assert np.array_equal(best, g["best"]) and best[0] == 227 != init             # the search moved off its starting point
    assert np.array_equal(C.fold(lf, 227), g["avg"]) and np.array_equal(C.fold_ordered(lf, 227), g["avg"])
    for P in (2, 3, 207, 250, 1033, 1034, 2067):
        assert np.array_equal(C.fold(lf, P), C.fold_ordered(lf, P)), P
    # P == 1: numpy coalesces the (V, 1) array into one contiguous run and sums it pairwise; the ordered sum is bounded against it
    assert abs(C.fold(lf, 1)[0] - C.fold_ordered(lf, 1)[0]) <= C.fold_bound_p1(lf)
    assert float(g["cycle_duration"]) == 227 * 128 / 22050 and float(g["rpm_measured"]) == 60.0 / (227 * 128 / 22050)
    assert str(g["printed"][0]).startswith("Best cycle length: 227.0")


def test_restated_tracker_reproduces_the_reference_track(g, pilot_db):
    """the band / argmax / parabola restatement on the reference's float64 dB spectrogram gives its track; on the float32 dB the
    kernels read, the track moves by float32 noise through the parabola only"""
    db64, db32 = pilot_db
    n = len(g["freqs"])
    assert (int(g["frame_0"]), int(g["frame_1"]), n) == (0, 2067, 2067) and db64.shape == (2068, 8193)
    trail = np.full(n, float(g["pilot_hz"]))
    f64, status, _ = C.track(db64, 0, trail, 16384, int(g["sr"]), int(g["tolerance_st"]) / 12, 0)
    assert status == 0 and np.allclose(f64, g["freqs"], rtol=1e-12, atol=0)
    f32, status, _ = C.track(db32, 0, trail, 16384, int(g["sr"]), int(g["tolerance_st"]) / 12, 0)
    assert status == 0 and np.max(np.abs(f32 - g["freqs"])) < 1e-4


def test_fixture_preconditions(g, pilot_db):
    """What the end-to-end GPU test leans on: a winner that float32 noise cannot unseat, and in every frame a strict band maximum
    whose parabola is well conditioned (denominator >= 1000 float32 ulps of the peak value)."""
    _, db32 = pilot_db
    deltas = np.sort(g["results"][:, 1])[::-1]
    assert deltas[0] - deltas[1] >= 100 * C.MARGIN_AVG, (deltas[0] - deltas[1], C.MARGIN_AVG)
    _, _, seen = C.track(db32, 0, np.full(2067, 700.0), 16384, 22050, 10 / 12, 0)
    worst = np.inf
    for i, (NL, NU, arg) in enumerate(seen):
        row = db32[i]
        assert (NL, NU) == (292, 927)
        assert np.sum(row[NL:NU] == row[arg]) == 1 and row[arg - 1] < row[arg] > row[arg + 1], i
        D = abs(np.float64(row[arg - 1]) - 2.0 * np.float64(row[arg]) + np.float64(row[arg + 1]))
        worst = min(worst, D / np.spacing(np.float32(abs(row[arg]))))
    assert worst >= 1000, worst


def test_band_restatement_edges():
    assert C.band_limits(700.0, 10 / 12, 16384, 22050, 8193) == (292, 927, False)
    assert C.band_limits(10.0, 0.1, 1024, 44100, 513) == (-1, 3, False)            # widened below bin 0: the empty slice
    assert C.band_limits(300.0, 0.2 / 12, 256, 48000, 129) == (0, 4, False)             # a band that starts on bin 0
    NL, NU, past = C.band_limits(23990.0, 0.001, 256, 48000, 129)                  # both edges capped at bins - 1, widened past the end
    assert (NL, NU, past) == (126, 129, True)
    row = np.array([1, 2, 5, 3, 1], dtype=np.float32)
    assert C.peak(row, 1, 5, False, 8, 8.0) == (0.5 * (2.0 - 3.0) / (2.0 - 10.0 + 3.0) + 2.0, 0)
    assert C.peak(row[::-1].copy(), 0, 5, False, 8, 8.0)[0] == 0.5 * (3.0 - 2.0) / (3.0 - 10.0 + 2.0) + 2.0
    assert C.peak(np.array([9, 2, 1, 1, 3], dtype=np.float32), 0, 4, False, 8, 8.0) == (0.5 * (3.0 - 2.0) / (3.0 - 18.0 + 2.0), 0)   # row[-1] is the left neighbour
    assert C.peak(row, 1, 2, False, 8, 8.0) == (1.0, 0)                            # the band's edge is no peak: the integer bin
    assert C.peak(np.array([1, 2, 3, 4, 5], dtype=np.float32), 1, 5, False, 8, 8.0) == (4.0, 2)
    assert C.peak(row, -1, 3, False, 8, 8.0) == (None, 1) and C.peak(row, 2, 5, True, 8, 8.0) == (2.0, 4)


def test_host_parts_of_the_module(g, monkeypatch):
    import torch
    assert W.default_hop(16384) == 128 and W.default_hop(4096) == 32
    assert W.candidate_range(229, 0.1) == (207, 44, 22) and W.candidate_range(229) == (207, 44, 22)
    assert W.candidate_range(9, 0.1) == (9, 0, 0) and W.candidate_range(459, 0.1) == (414, 90, 45)
    assert W.channel_index("L", 1) == 0 and W.channel_index("R", 2) == 1 and W.channel_index(1, 2) == 1
    with pytest.raises(ValueError):
        W.channel_index("R", 1)
    assert W.fused_supported(16384) and W.fused_supported(4096, 4) and not W.fused_supported(32768) and not W.fused_supported(1000)
    # first occurrence on ties, as np.argmax
    assert W.best_cycle(np.array([[5, 0.1], [6, 0.3], [7, 0.3], [8, 0.2]])) == (6, 0.3)
    with pytest.raises(ValueError):
        W.best_cycle(np.empty((0, 2)))                                              # d == 0: the reference's argmax of nothing
    # analyse's wiring on the golden track, the device parts replaced by numpy: the reference's figures to the bit
    seen = {}

    def fake_track(signal, sr, trail, fft_size, hop, tolerance_st, channel, db, mode, **kw):
        seen.update(sr=sr, trail=trail, fft_size=fft_size, hop=hop, tolerance_st=tolerance_st, channel=channel, db=db, mode=mode)
        return g["times"].copy(), g["freqs"].copy(), 0, len(g["freqs"])

    def fake_fold(v, p_first, n_cand, want_avg, dev):
        seen.setdefault("folds", []).append((p_first, n_cand, want_avg))
        rows = [C.fold(np.asarray(v), p_first + c) for c in range(n_cand)]
        avg = np.full((n_cand, p_first + n_cand - 1), np.nan)
        for c, r in enumerate(rows):
            avg[c, :len(r)] = r
        return torch.from_numpy(avg), torch.from_numpy(np.array([r.max() - r.min() for r in rows]))
    monkeypatch.setattr(W._dev, "device_index", lambda device=None: 0)
    monkeypatch.setattr(W._dev, "to_dev", lambda a, dtype, dev: a)
    monkeypatch.setattr(W, "pilot_track", fake_track)
    monkeypatch.setattr(W, "_fold_dev", fake_fold)
    stereo = np.zeros((264600, 2), dtype=np.float32)
    res = W.analyse(stereo, sr=22050, channel="R")
    assert seen["hop"] == 128 and seen["fft_size"] == 16384 and seen["channel"] == 1 and seen["db"] is True and seen["mode"] == "Peak"
    assert seen["trail"] == [(0.0, 700.0), (264600 / 22050, 700.0)] and seen["tolerance_st"] == 10
    assert seen["folds"] == [(207, 44, False), (227, 1, True)]
    assert res.frames_per_rotation == 227 and res.delta == float(g["best"][1]) and np.array_equal(res.results, g["results"])
    assert res.cycle_duration == float(g["cycle_duration"]) and res.rpm_measured == float(g["rpm_measured"])
    assert np.array_equal(res.avg, g["avg"]) and np.array_equal(res.freqs, g["freqs"])
    with pytest.raises(ValueError):
        W.analyse(stereo[:, 0], sr=22050, channel="R")
    with pytest.raises(ValueError):
        W.analyse(stereo)                                                           # a signal without its rate
    # speed_curve: one point per traced frame, the cycle tiled, geometric mean 1 over a cycle
    curve = W.speed_curve(res, 22050, 128)
    P = res.frames_per_rotation
    assert curve.shape == (2067, 2) and np.array_equal(curve[:, 0], g["times"])
    assert np.array_equal(curve[P:2 * P, 1], curve[:P, 1]) and np.array_equal(curve[8 * P:, 1], curve[:2067 - 8 * P, 1])
    assert abs(np.mean(np.log2(curve[:P, 1]))) < 1e-15
    assert np.array_equal(curve[:P, 1], np.power(2.0, g["avg"] - np.mean(g["avg"])))
    assert 0.008 < curve[:, 1].max() - curve[:, 1].min() < 0.012                 # the +-0.5 % of the pilot, its harmonic on top
    with pytest.raises(ValueError):
        W.speed_curve(res, 22050, 256)
    rep = W.report(res)
    assert rep["delta_semitones"] == rep["delta_octaves"] * 12 and rep["frames_per_rotation"] == 227


P8 = ctypes.c_void_p(8)


def _peak(L, x=P8, n=40000, stride=1, n_fft=1024, hop=128, zp=1, win=P8, f0=0, count=10, freqs=P8, sr=44100.0, tol=0.5, mode=0, db=0,
          status=P8):
    return L.par_stft_track_peak_f64(0, x, n, stride, n_fft, hop, zp, win, f0, count, freqs, sr, tol, mode, db, status, None)


def test_track_peak_argument_errors_before_any_device_call():
    from pyaudiorestoration_amd import _lib
    L = _lib.lib()
    frames = L.par_stft_frames(40000, 1024, 128)
    for kw in (dict(x=None), dict(win=None), dict(freqs=None), dict(status=None), dict(n=0), dict(hop=0), dict(zp=0), dict(n_fft=1),
               dict(stride=0), dict(count=-1), dict(f0=-1), dict(f0=frames - 9), dict(count=frames + 1), dict(f0=2 ** 62, count=2 ** 62),
               dict(mode=2), dict(mode=-1), dict(db=2), dict(db=-1)):
        assert _peak(L, **kw) == 1, kw
        assert "par_stft_track_peak_f64" in _lib.last_error()
    for kw in (dict(n_fft=1000), dict(n_fft=8), dict(n_fft=32768), dict(n_fft=16384, zp=2), dict(n_fft=1022), dict(n_fft=6, zp=4)):
        assert _peak(L, count=1, **kw) == 3 and "power of two" in _lib.last_error(), kw
        with pytest.raises(_lib.ParUnsupported):
            _lib.check(3)
    assert _peak(L, count=0) == 0 and _peak(L, count=0, f0=frames) == 0              # nothing to trace: no device call either


def test_cycle_fold_argument_errors_before_any_device_call():
    from pyaudiorestoration_amd import _lib
    L = _lib.lib()

    def fold(v=P8, count=1000, p_first=10, n_cand=5, avg=P8, pitch=14, delta=P8):
        return L.par_cycle_fold_f64(0, v, count, p_first, n_cand, avg, pitch, delta, None)
    for kw in (dict(v=None), dict(delta=None), dict(p_first=0), dict(p_first=-3), dict(n_cand=0), dict(count=13), dict(count=-1),
               dict(p_first=1000, n_cand=2), dict(p_first=2 ** 31 - 1, n_cand=2 ** 31 - 1), dict(pitch=13)):
        assert fold(**kw) == 1 and "par_cycle_fold_f64" in _lib.last_error(), kw
