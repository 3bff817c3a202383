"""Float64 numpy restatement of what the cyclic wow kernels compute, for test_cyclic_cpu.py and the GPU tests.

* band / argmax / parabola of PeakTracker and PeakTrackTracker (util/wow_detection.py:97-139, 294-327; parabolic of
  util/correlation.py:42-46) on a GIVEN float32 spectrogram [frames][bins]: the GPU tests hand it the spectrogram par_stft_f32
  mode 1 wrote for the same device samples, so the transform is not part of the comparison;
* get_avg and the search loop of experiments/cyclic_wow.py:9-27, 50-64.

Status bits as the kernels report them: 1 empty band, 2 peak on the last bin, 4 band past the last bin."""
import numpy as np

# End-to-end margins against the reference's track and fold on tests/golden/cyclic_pilot.wav (test_cyclic_gpu.py).  The yardstick
# is the COMPOSED path at the parent's kernels (K_stft mode 1, float32 dB, par_track_peak_f64), measured on the MI355X against
# tests/golden/cyclic.npz: largest |freqs - reference| in Hz and largest |avg - reference| in octaves.  The fused kernel is
# allowed four times that: it is float32-transform noise through a parabola and varies by frame.
COMPOSED_DEV_FREQS = 4.1e-6        # measured 4.050e-6 Hz
COMPOSED_DEV_AVG = 3.6e-9          # measured 3.570e-9 octaves
MARGIN_FREQS = 4 * COMPOSED_DEV_FREQS
MARGIN_AVG = 4 * COMPOSED_DEV_AVG


def to_db32(mag):
    """the float32 dB spectrogram: (float)(20 log10((double) m))"""
    return (20.0 * np.log10(np.asarray(mag, dtype=np.float32).astype(np.float64))).astype(np.float32)


def band_limits(freq, tol, fft_size, sr, bins):
    """-> (NL, NU, past_end): freq_plus_tolerance, set_bin_limits with min_bins = 4, NU clipped to the spectrum"""
    lf = np.log2(np.float64(freq))
    fL, fU = max(1.0, float(np.power(2.0, lf - tol))), min(sr / 2, float(np.power(2.0, lf + tol)))

    def to_bin(f):
        return max(1, min(bins - 1, int(round(f * fft_size / sr))))
    NL, NU = to_bin(fL), to_bin(fU)
    while NU - NL < 4:
        NL -= 1
        NU += 1
    return NL, min(NU, bins), NU > bins


def peak(row, NL, NU, past_end, fft_size, sr):
    """get_peak on one frame `row` (float32[bins]) -> (Hz, status bits).  An empty band returns (None, 1)."""
    bins = len(row)
    if NL < 0 or NL >= NU:
        return None, 1
    arg = NL + int(np.argmax(row[NL:NU]))
    x = float(arg)
    if past_end:
        return x / fft_size * sr, 4
    if arg == bins - 1:
        return x / fft_size * sr, 2
    fm, f0, fp = (np.float64(row[k]) for k in (arg - 1, arg, arg + 1))         # row[-1] at arg == 0: Python's wrap
    if fm < f0 > fp:
        x = 0.5 * (fm - fp) / (fm - 2.0 * f0 + fp) + x
    return x / fft_size * sr, 0


def track(spec, frame_0, trail_freqs, fft_size, sr, tol, mode):
    """PeakTracker (mode 0) / PeakTrackTracker (mode 1) over frames frame_0 + i of spec [frames][bins] float32, before NaN
    patching -> (freqs float64, status bits OR-ed, [(NL, NU, arg) per frame]).  A frame with an empty band keeps its trail value."""
    out = np.array(trail_freqs, dtype=np.float64)
    bins = spec.shape[1]
    status, seen = 0, []
    for i in range(len(out)):
        if mode == 0:
            NL, NU, past = band_limits(out[i], tol, fft_size, sr, bins)
        else:
            NL, NU, past = band_limits(trail_freqs[0], tol / 2 if i > 2 else tol, fft_size, sr, bins)
        f, st = peak(spec[frame_0 + i], NL, NU, past, fft_size, sr)
        status |= st
        if f is not None:
            out[i] = f
        seen.append((NL, NU, None if f is None else NL + int(np.argmax(spec[frame_0 + i][NL:NU]))))
    return out, status, seen


def parabola_bound(row, arg, fft_size, sr):
    """The db = 1 bound of the issue: 2 * 3u / |D| * sr / fft_size with u one float32 ulp of the largest of the three dB values
    and D = a - 2b + c (first-order bound of the parabola under one-ulp perturbations at a true peak, doubled for the second
    order)."""
    a, b, c = (np.float64(row[k]) for k in (arg - 1, arg, arg + 1))
    u = np.float64(np.spacing(np.float32(max(abs(a), abs(b), abs(c)))))
    return 2.0 * 3.0 * u / abs(a - 2.0 * b + c) * sr / fft_size


def fold(v, P):
    """get_avg: np.mean(np.split(v[:V * P], V), axis=0), V = len(v) // P"""
    V = len(v) // P
    return np.mean(np.split(np.asarray(v, dtype=np.float64)[:V * P], V), axis=0)


def fold_ordered(v, P):
    """the same, with the order spelled out: views added one after the other from view 0, one division by V.  Equal to fold()
    bit for bit for P >= 2; at P == 1 numpy coalesces the (V, 1) array into one contiguous run and sums it PAIRWISE, and the two
    differ within fold_bound_p1."""
    v = np.asarray(v, dtype=np.float64)
    V = len(v) // P
    s = v[:P].copy()
    for w in range(1, V):
        s = s + v[w * P:(w + 1) * P]
    return s / V


def fold_bound_p1(v):
    """|ordered - pairwise| at P == 1: each is within (V - 1) 2^-53 sum|v| of the exact sum, then both are divided by V"""
    v = np.asarray(v, dtype=np.float64)
    return 2.0 * (len(v) - 1) * 2.0 ** -53 * np.sum(np.abs(v)) / len(v)


def search(v, frames_init, tolerance):
    """the search loop -> results (2 d, 2)"""
    d = int(frames_init * tolerance)
    results = np.empty((d * 2, 2))
    for i in range(-d, d):
        avg = fold(v, frames_init + i)
        results[d + i] = (frames_init + i, np.max(avg) - np.min(avg))
    return results


def tone(n, sr, f, amp=0.5, noise=0.0, seed=0):
    """float32 tone of instantaneous frequency f (scalar or per sample)"""
    f = np.broadcast_to(np.asarray(f, dtype=np.float64), (n,))
    x = amp * np.sin(2 * np.pi * np.cumsum(f) / sr)
    if noise:
        x = x + noise * np.random.default_rng(seed).standard_normal(n)
    return x.astype(np.float32)
