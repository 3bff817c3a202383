"""K_track (csrc/track.hip) against oracle.oracle_np.TRACKERS where test_hip_parity.py's stationary pilot does not reach: bands
that move from frame to frame, that cross the 64-bin width between k_track_cog's two loops, that reach bin 0, trails that start on
0 / end past the file / span one frame, spectrogram rows with padding, and k_track_peak_refined against a float64 spectrum of the
same float32 frames, at the signal's ends, with zero extension, with fewer samples than threads and with a hop off the grid.

Oracle and tracker read the SAME numbers: fourier.get_mag's device spectrogram, copied to the host and widened to float64 for the
oracle (with float32 input its parabolic() would run in float32).  tests/test_tracker_inputs_cpu.py proves that no band edge of
these inputs sits within 1e-6 bins of a rounding cliff, so a band that differs here is a kernel error; each case re-asserts its
row of those preconditions on the spectrogram it actually used.  pytest -s prints the measured errors (NOTES.md, K_track)."""
import numpy as np
import pytest
import scipy.signal

import tracker_inputs as T
from oracle import oracle_np as O

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]     # the oracle's log2(0) on bin 0

SAME_MAG_TOL = 1e-9        # float64 on both sides of the same magnitudes (test_correlation_tracker_wide_and_clipped_bands' bound)
REFINED_TOL = 2.6e-14      # k_track_peak_refined against numpy's float64 rfft of the same float32 frames: 10 x the worst of the
#                            eight runs below (2.54e-15: Peak Track at 1024 / 100 / zeropad 2, whose fixed band the glide leaves, so it
#                            reads magnitudes 1e-4 of the peak; Peak itself <= 4.2e-16) -- six orders under the 2e-8 the golden grants


def relerr(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size == 0:
        return 0.0
    return float(np.float64(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300))


@pytest.fixture(scope="module")
def par():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pyaudiorestoration_amd import fourier, wow_detection

    class P:
        pass
    p = P()
    p.torch, p.fourier, p.wow = torch, fourier, wow_detection
    return p


@pytest.fixture(scope="module")
def spectra(par):
    """case -> (signal on the device, device spectrogram, the same magnitudes as float64 on the host); computed once per case."""
    cache = {}

    def get(c):
        if c.name not in cache:
            xt = par.torch.from_numpy(np.array(c.x)).cuda()
            mag_t = par.fourier.get_mag(xt, c.n_fft, c.hop, T.WINDOW, c.zeropad)
            host = mag_t.cpu().numpy().astype(np.float64)
            host.setflags(write=False)
            cache[c.name] = (xt, mag_t, host)
        return cache[c.name]
    return get


def run(par, name, spec, c, **kw):
    return par.wow.wow_detectors[name](spec, c.x[:, None], c.trail, c.fft_size, c.hop, c.sr, c.tol, "Linear", **kw)


def compare_with_oracle(par, c, mag_t, host, trackers=T.TRACKERS):
    worst = {}
    for name in trackers:
        want_t, want_f = O.TRACKERS[name](host, c.trail, c.fft_size, c.hop, c.sr, c.tol)
        tr = run(par, name, mag_t, c)
        assert np.array_equal(tr.times, want_t), (c, name)
        assert np.isfinite(want_f).all() and np.isfinite(tr.freqs).all(), (c, name)
        worst[name] = relerr(tr.freqs, want_f)
        assert worst[name] < SAME_MAG_TOL, (c, name, worst[name])
    return worst


@pytest.mark.parametrize("name", T.NAMED + T.TRAIL_SHAPES)
def test_spectrogram_trackers_on_moving_bands(par, spectra, name):
    c = T.case(name)
    _, mag_t, host = spectra(c)
    assert host.shape[0] == c.bins
    stats, raw = T.assert_paths(name, host, c)             # this spectrogram drives the kernel down the paths the case is for
    assert T.cliff_margin(host, c) >= T.CLIFF_MARGIN
    trackers = T.TRACKERS
    if name == "bin0":
        # Correlation's band starts on bin 0: log2(0) poisons every frame and patching an all-NaN line raises on both sides
        trackers = T.TRACKERS[:3]
        with pytest.raises(ValueError) as want:
            O.TRACKERS["Correlation"](host, c.trail, c.fft_size, c.hop, c.sr, c.tol)
        with pytest.raises(ValueError) as got:
            run(par, "Correlation", mag_t, c)
        assert "sample points is empty" in str(want.value) and "sample points is empty" in str(got.value)
    worst = compare_with_oracle(par, c, mag_t, host, trackers)
    print(f"\n{name}: {stats}, NaN frames {np.isnan(raw).nonzero()[0].tolist()}, relative errors {worst}")


@pytest.mark.parametrize("seed", T.SWEEP_SEEDS)
def test_seeded_sweep_against_the_oracle(par, spectra, seed):
    c = T.sweep_case(seed)
    _, mag_t, host = spectra(c)
    assert T.cliff_margin(host, c) >= T.CLIFF_MARGIN
    worst = compare_with_oracle(par, c, mag_t, host)       # every (seed, tracker) pair compares: nothing is skipped
    print(f"\nseed {seed}: sr {c.sr} n_fft {c.n_fft} hop {c.hop} tol {c.tol}, relative errors {worst}")


@pytest.mark.parametrize("name", ["glide3", "bin0"])
def test_pitched_rows_with_sentinels(par, spectra, name):
    """Rows `bins + 37` floats apart, the padding filled with 3e38: an index that leaves its row reads a value that wins every
    argmax and swamps every centroid."""
    c = T.case(name)
    _, mag_t, _ = spectra(c)
    t = par.torch
    packed = mag_t.T.contiguous()                           # [frames][bins]
    frames, bins = packed.shape
    buf = t.full((frames, bins + 37), 3e38, dtype=t.float32, device=packed.device)
    buf[:, :bins] = packed
    pitched = buf[:, :bins].T
    taken = par.wow.spectrum_to_device(pitched)
    assert taken.stride(0) == bins + 37 and taken.stride(1) == 1 and taken.data_ptr() == buf.data_ptr()      # zero-copy
    assert par.wow.spectrum_to_device(packed.T).stride(0) == bins
    for tracker in T.TRACKERS[:3]:
        a, b = run(par, tracker, pitched, c), run(par, tracker, packed.T, c)
        assert np.array_equal(a.times, b.times) and np.array_equal(a.freqs, b.freqs), (name, tracker, relerr(a.freqs, b.freqs))
    assert bool((buf[:, bins:] == 3e38).all())


refined_worst = {}


@pytest.mark.parametrize("n_fft,hop,zp,dur", T.REFINED)
def test_refined_peak_against_float64_spectrum(par, spectra, monkeypatch, n_fft, hop, zp, dur):
    """k_track_peak_refined evaluates the DFT of the reference's float32 frames in float64; so does numpy's rfft of the same frames
    (tracker_inputs.float64_mag).  Both sides are float64 evaluations of one set of numbers: the bound is 10 x the worst error
    measured over these eight runs (four transforms, contiguous and strided channel), for libm and reduction order."""
    c = T.refined_case(n_fft, hop, zp, dur)
    xt, mag_t, _ = spectra(c)
    ref = T.float64_mag(c)
    assert ref.shape == tuple(mag_t.shape) and T.cliff_margin(ref, c) >= T.CLIFF_MARGIN
    t = par.torch
    win_t = t.from_numpy(scipy.signal.get_window(T.WINDOW, n_fft).astype(np.float32)).cuda()
    inter = t.stack((xt, xt.flip(0)), dim=1).contiguous()
    L = par.wow._lib.lib()
    calls = []
    abi = L.par_track_peak_refined_f64
    monkeypatch.setattr(L, "par_track_peak_refined_f64", lambda *a: calls.append(a) or abi(*a))
    for view in (xt, inter.reshape(-1)[0::2]):
        refine = {"x": view, "n_fft": n_fft, "zeropad": zp, "window": win_t}
        for name in ("Peak", "Peak Track"):
            want_t, want_f = O.TRACKERS[name](ref, c.trail, c.fft_size, c.hop, c.sr, c.tol)
            del calls[:]
            tr = run(par, name, mag_t, c, refine=refine)
            assert len(calls) == 1 and calls[0][3] == view.stride(0)            # _trace_refined was taken, on this view
            plain = run(par, name, mag_t, c)
            assert len(calls) == 1 and not np.array_equal(tr.freqs, plain.freqs)
            assert np.array_equal(tr.times, want_t) and len(want_t) == int(dur * c.sr / hop)
            err = relerr(tr.freqs, want_f)
            refined_worst[(n_fft, hop, zp, view.stride(0), name)] = err
            print(f"\nrefined {name} n_fft {n_fft} hop {hop} zeropad {zp} stride {view.stride(0)}: {err:.3e} "
                  f"(float32 spectrogram path: {relerr(plain.freqs, want_f):.3e})")
            assert err < REFINED_TOL, (name, n_fft, hop, zp, err)
    print(f"worst refined error so far: {max(refined_worst.values()):.3e}")


def test_refined_error_reports(par, monkeypatch):
    """The refined path raises what the spectrogram path raises in test_tracker_error_behaviour_matches_reference -- by itself:
    the spectrogram path is taken away for the length of this test."""
    import inputs
    t = par.torch

    def no_fallback(*a, **k):
        raise AssertionError("the refined trace fell back to the spectrogram")
    monkeypatch.setattr(par.wow.Track, "_trace_on_device", no_fallback)
    sr, n_fft, hop = 192000, 256, 64
    win_t = t.from_numpy(scipy.signal.get_window(T.WINDOW, n_fft).astype(np.float32)).cuda()

    def trace(name, x, xt, mag, trail, tol):
        refine = {"x": xt, "n_fft": n_fft, "zeropad": 1, "window": win_t}
        return par.wow.wow_detectors[name](mag, x[:, None], list(trail), n_fft, hop, sr, tol, "Linear", refine=refine)

    x = inputs.sine(60000, 800.0, sr, 0.5)
    xt = t.from_numpy(x).cuda()
    mag = par.fourier.get_mag(xt, n_fft, hop, T.WINDOW, 1)
    low = [(0.05, 800.0), (0.25, 800.0)]                                 # 800 Hz = bin 1.07 of a 750 Hz grid: empty band
    for name in ("Peak", "Peak Track"):
        with pytest.raises(ValueError, match="par_track_peak_refined_f64"):
            trace(name, x, xt, mag, low, 0.5)
    ny = (0.5 * np.cos(np.pi * np.arange(60000))).astype(np.float32)
    nyt = t.from_numpy(ny).cuda()
    mag_ny = par.fourier.get_mag(nyt, n_fft, hop, T.WINDOW, 1)
    top = [(0.05, 95000.0), (0.25, 95000.0)]                            # the band ends ON the last bin with the peak there
    with pytest.raises(IndexError, match="par_track_peak_refined_f64"):
        trace("Peak Track", ny, nyt, mag_ny, top, 0.5)
    past = [(0.05, 95900.0), (0.25, 95900.0)]                           # the band is widened PAST the last bin
    for name in ("Peak", "Peak Track"):
        with pytest.raises(ValueError, match="par_track_peak_refined_f64"):
            trace(name, ny, nyt, mag_ny, past, 0.01)
    one_frame = [(0.1000, 4000.0), (0.1001, 4000.0)]
    tr = trace("Peak", x, xt, mag, one_frame, 0.5)
    assert len(tr.freqs) == 0 and len(tr.times) == 0
    with pytest.raises(IndexError):
        trace("Peak Track", x, xt, mag, one_frame, 0.5)
