"""Seeded inputs and float64 oracles for the tape-sync tool's azimuth mode (pytapesynch_gui.py:210-238): the batched delay
search par_find_delay_batch_f64, the window gather par_gather_windows_f64 and pipeline.azimuth_windows / azimuth_line /
azimuth_reject / lag_curve_from_markers(azimuths=...).  No device code is imported here: tests/test_azimuth_cpu.py proves the
preconditions of every builder with the oracles alone, tests/test_azimuth_gpu.py holds the kernels to them."""
from collections import namedtuple

import numpy as np
import scipy.ndimage
import scipy.signal

import xcorr_inputs as X

REJECT = 0.1
SAFETY = 4.0                            # the margin tests/test_xcorr_gpu.py puts on xcorr_inputs.delay_bounds
FILTER_TOL = 1e-9                       # K_sosfiltfilt's batched form against scipy's sosfiltfilt on the WIDE order-3 band-passes of this flow:
                                        # max |y - y_scipy| <= FILTER_TOL max |y_scipy|.  The kernels are pinned to the long-double oracle at
                                        # filt_inputs.R x scipy's own error (test_filt_kernels_gpu.py); on these bands that error is ~1e-14, so
                                        # the figure has three decades of slack (test_filt_cpu.py::test_azimuth_flow_filter_premise).  It does
                                        # NOT hold on bands near z = 1 (1-2 Hz at 44.1 kHz: scipy itself is 4e-8 from the oracle)
CEILING = 1e-6                          # every case is built so that its whole bound stays below this (samples; correlation units)


# --------------------------------------------------------------------------------------------------- get_signal, literally

def get_signal(signal, sr, t0, t1):
    """Spectrum.get_signal (util/spectrum.py:158-171) on a 1-D signal -> (window, (start, length, pad_l, pad_r)).  The slice keeps
    Python's meaning of a negative start."""
    sample0 = int(t0 * sr)
    sample1 = int(t1 * sr)
    pad_l = 0
    pad_r = 0
    if sample0 < 0:
        pad_l = abs(sample0)
    if sample1 > len(signal):
        pad_r = sample1 - len(signal)
    sig = signal[sample0:sample1]
    start = slice(sample0, sample1).indices(len(signal))[0]
    return np.pad(sig, (pad_l, pad_r), "constant", constant_values=0), (start, len(sig), pad_l, pad_r)


def window_pair(ref, src, sr, x, d, dur):
    """the two get_signal_around calls of Canvas.correlate_sources(x - dur, x + dur, d, ...) (pytapesynch_gui.py:108-125)"""
    t0, t1 = x - dur, x + dur
    t_center = (t0 + t1) / 2
    t_width = (t1 - t0) / 2
    a, ga = get_signal(ref, sr, t_center - t_width, t_center + t_width)
    c = t_center - d
    b, gb = get_signal(src, sr, c - t_width, c + t_width)
    return a, b, ga, gb


def windows_of(ref, src, sr, t0, t1, lag_curve, dur, overlap):
    """the Alt branch's loop header (:218-231) -> (sample_times, sample_lags, [(a, b, geom_a, geom_b)])"""
    sample_times = np.arange(t0, t1, dur / overlap)
    if not len(sample_times):
        return sample_times, np.zeros(0), []
    lag_curve = np.asarray(lag_curve, dtype=np.float64)
    sample_lags = np.interp(sample_times, lag_curve[:, 0], lag_curve[:, 1])
    return sample_times, sample_lags, [window_pair(ref, src, sr, x, d, dur) for x, d in zip(sample_times, sample_lags)]


Geometry = namedtuple("Geometry", "name len_ref len_src sr t0 t1 lag_curve dur overlap")


def geometry_cases():
    sr, n = 8000, 20000                                   # 2.5 s
    flat = lambda d: np.array([[0.0, d], [10.0, d]])
    return [
        Geometry("inside", n, n - 77, sr, 0.5003, 1.0, np.array([[0.0, 0.011], [2.0, 0.0173]]), 0.05003, 4),      # 800.48 samples
        Geometry("over_the_end", n, n - 77, sr, 2.3, 2.56, flat(0.0031), 0.05, 4),
        Geometry("before_0_ref_only", n, n, sr, 0.0101, 0.2, flat(-0.1), 0.05, 4),
        Geometry("before_0_src_only", n, n, sr, 0.0601, 0.2, flat(0.1), 0.05, 4),
        Geometry("before_0_both", n, n, sr, 0.0, 0.2, flat(0.0), 0.05, 4),
        Geometry("int_truncates_from_below", n, n, sr, 0.05 - 0.5 / sr, 0.2, flat(0.0), 0.05, 4),
        Geometry("src_past_the_end", n, n, sr, 1.0, 1.2, flat(-3.0), 0.05, 4),
        Geometry("src_before_the_start", n, n, sr, 1.0, 1.2, flat(3.0), 0.05, 4),        # negative indices: a slice from the END
        Geometry("src_far_before_the_start", n, n, sr, 1.0, 1.2, flat(5.0), 0.05, 4),
        Geometry("short_file", 450, 470, sr, 0.0, 0.06, flat(0.001), 0.05, 4),      # len - |sample0| < sample1: the wrapped slice is not empty
        Geometry("empty", n, n, sr, 1.0, 1.0, flat(0.0), 0.05, 4),
        Geometry("empty_reversed", n, n, sr, 1.0, 0.9, flat(0.0), 0.05, 4),
    ]


def geometry_signals(g, seed=0):
    rng = np.random.default_rng([81, g.len_ref, g.len_src, seed])
    return rng.standard_normal(g.len_ref).astype(np.float32), rng.standard_normal(g.len_src).astype(np.float32)


# ------------------------------------------------------------------------------------------------------ per-window oracle

def oracle_window(a, b, sr, lower, upper, ignore_phase=False):
    """float64 oracle of one window: order-3 zero-phase band-pass on both, Hann windows, xcorr_inputs.oracle_delay.  A window of
    zeros has norm 0: the reference divides by it and carries NaN through -> None.
    -> (oracle or None, windowed rows fa, fb, (delay bound, corr bound) of flow_bounds)"""
    from oracle import oracle_np as O
    ya = np.array(O.butter_bandpass_filter(np.asarray(a, dtype=np.float64), lower, upper, sr, order=3), dtype=np.float64)
    yb = np.array(O.butter_bandpass_filter(np.asarray(b, dtype=np.float64), lower, upper, sr, order=3), dtype=np.float64)
    wa, wb = scipy.signal.get_window("hann", len(ya)), scipy.signal.get_window("hann", len(yb))
    fa, fb = ya * wa, yb * wb
    if not np.any(fa) or not np.any(fb):
        return None, fa, fb, None
    o = X.oracle_delay(fa, fb, ignore_phase)
    return o, fa, fb, flow_bounds(o, ya, yb, wa, wb)


def flow_bounds(o, ya, yb, wa, wb):
    """(|d delay| in samples, |d corr|) allowed between the device flow (K_sosfiltfilt, Hann, delay search) and the float64 oracle of
    one window.  Two terms, both through xcorr_inputs.delay_bounds' first-order propagation 3 df / D and 1.25 df + 0.75 |fm - fp| df / D:
      * the float64 dot products, df = delta_f(nb), at the SAFETY margin tests/test_xcorr_gpu.py uses;
      * the filter.  On this flow's wide band-passes K_sosfiltfilt is within |e_i| <= FILTER_TOL max |y| of scipy (see FILTER_TOL:
        the oracle pin gives 2e-13, the figure is kept at 1e-9), so the windowed row moves by
        ||e w|| <= FILTER_TOL max |y| ||w||, the normalised row u = x / ||x|| by at most twice that over ||y w||, and a correlation
        value <u_a, u_b> of unit rows by at most the sum of the two rows' moves: df = 2 (eps_a + eps_b)."""
    D = abs(o.fm - 2.0 * o.f0 + o.fp)
    eps = [FILTER_TOL * np.max(np.abs(y)) * np.linalg.norm(w) / np.linalg.norm(y * w) for y, w in ((ya, wa), (yb, wb))]
    df = SAFETY * X.delta_f(len(yb)) + 2.0 * (eps[0] + eps[1])
    return 3.0 * df / D, 1.25 * df + 0.75 * abs(o.fm - o.fp) * df / D


def golden_window_bounds(g, ref, src):
    """[(oracle, flow_bounds)] for every window of tests/golden/azimuth.npz, cut out of the two files by the stored geometry"""
    sr, lower, upper = int(g["sr"]), float(g["lower"]), float(g["upper"])
    cut = lambda sig, q: np.concatenate((np.zeros(q[2], sig.dtype), sig[q[0]:q[0] + q[1]], np.zeros(q[3], sig.dtype)))
    out = []
    for qa, qb in zip(g["ref_geom"], g["src_geom"]):
        o, _, _, flow = oracle_window(cut(ref, qa), cut(src, qb), sr, lower, upper)
        out.append((o, flow))
    return out


def reject_np(lags_raw, corrs, overlap, reject):
    """AzimuthLine.update_reject's three lines (util/markers.py:542-552)"""
    lags = np.array(lags_raw, dtype=np.float64)
    lags[np.abs(corrs) < reject] = np.nan
    nans = np.isnan(lags)
    idx = lambda z: z.nonzero()[0]
    lags[nans] = np.interp(idx(nans), idx(~nans), lags[~nans])
    size = overlap if overlap % 2 else overlap + 1
    return scipy.ndimage.median_filter(lags, size=size, footprint=None, output=None, mode='nearest', cval=0.0, origin=0)


# --------------------------------------------------------------------------------------------------- batch cases (test 1-5)

BATCH_SHAPES = ((1000, 1000), (1000, 999), (1000, 64), (4097, 4096), (4097, 4097))     # 8192 = exact fit, 8193 = first of 16 384
BATCH_WS = (1, 2, 37)
BATCH_KINDS = ("white", "narrow", "tone")


# The preconditions (tests/test_azimuth_cpu.py) decide which takes a shape can use.  signal_pair's narrow-band take (2e-4 .. 1.2e-3 of
# Nyquist) of 4096 samples has so flat a peak (|fm - 2 f0 + fp| ~ 1e-8) that 4 x delay_bounds is 1.4e-6 samples, above the 1e-6 the
# cases must stay under: the long shapes take the same construction with a band ten times as wide (the curvature grows with its
# square).  Seed 13 of the narrow take peaks ON the last lag at 1000 x 64 (the reference's IndexError, which test 4 covers with a
# row built for it): that row takes another seed.
NARROW_MAX_NB = 1000
RESEED = {(1000, 64, 13): 113}


def narrow_pair_wide(na, nb, seed=0):
    """xcorr_inputs.signal_pair("narrow", ...) with the band 2e-3 .. 1.2e-2 of Nyquist"""
    rng = np.random.default_rng([84, na, nb, seed])
    sos = scipy.signal.butter(2, [2e-3, 1.2e-2], btype="band", output="sos")
    src = scipy.signal.sosfilt(sos, rng.standard_normal(max(na, nb) + 64))
    return src[:na].copy(), 0.9 * src[17:17 + nb] + 0.01 * rng.standard_normal(nb)


def batch_rows(na, nb, W, seed=0):
    """W window pairs of one shape: white, narrow-band and tone takes in turn, every row its own seed"""
    a = np.empty((W, na))
    b = np.empty((W, nb))
    for w in range(W):
        kind, sd = BATCH_KINDS[w % 3], 1000 * seed + RESEED.get((na, nb, w), w)
        a[w], b[w] = narrow_pair_wide(na, nb, sd) if kind == "narrow" and nb > NARROW_MAX_NB else X.signal_pair(kind, na, nb, seed=sd)
    return a, b


def rival_batches():
    """{name: (a rows, b rows, special row, rival_case lags or None)}: a rival_case row between two ordinary rows of its shape"""
    out = {}
    for name, K, loud in (("K2", 2, 1), ("K32", 32, 16), ("plateau", 65, 40)):
        ra, rb, lags = X.rival_case(K, loud)
        n = len(ra)
        o1 = X.signal_pair("white", n, n, seed=K)
        o2 = X.signal_pair("tone", n, n, seed=K + 1)
        out[name] = (np.stack((o1[0], ra, o2[0])), np.stack((o1[1], rb, o2[1])), 1, lags, loud)
    return out


def status_batch(na=1000, nb=999):
    """five rows: ordinary, a peak on lag na - 1 (status 1), ordinary, all zeros (NaN, status 0), ordinary"""
    a, b = batch_rows(na, nb, 5, seed=3)
    a[1], b[1] = X.edge_case(na, nb, na - 1)
    a[3], b[3] = 0.0, 0.0
    return a, b, 1, 3


# ------------------------------------------------------------------------------------------------------ end to end (test 7)

E2E = dict(sr=8000, dur=0.05, overlap=4, lower=300.0, upper=3000.0, t0=0.0203, t1=0.5203, n_ref=4400, n_src=4300,
           lag_curve=np.array([[0.0, 0.0030], [1.0, 0.0036]]))


def e2e_files(seed=0):
    """broadband noise low-passed like test_correlate_sources_flow's; the source is the reference delayed by a slowly varying
    fractional lag (3.4 ms +- 0.4 ms over the file), 2-channel float32 files with the take in channel 1 / channel 0"""
    p = E2E
    rng = np.random.default_rng([82, seed])
    base = np.convolve(rng.standard_normal(p["n_ref"] + 800), np.hanning(9) / 4, mode="same")
    k = np.arange(len(base))
    ref = base[400:400 + p["n_ref"]]
    t = np.arange(p["n_src"]) / p["sr"]
    lag = 0.0034 + 0.0004 * np.sin(2.0 * np.pi * t / 0.6)
    src = 0.8 * np.interp(np.arange(p["n_src"]) + 400 + lag * p["sr"], k, base) + 0.01 * rng.standard_normal(p["n_src"])
    ref2 = np.stack((rng.standard_normal(p["n_ref"]), ref), axis=-1).astype(np.float32)
    src2 = np.stack((src, rng.standard_normal(p["n_src"])), axis=-1).astype(np.float32)
    return ref2, src2, 1, 0
