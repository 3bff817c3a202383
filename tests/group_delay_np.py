"""Float64 host statements for the group-delay flow (pyaudiorestoration_amd/group_delay.py, par_find_delay_sect_f64):

  * fixture_signals      the seeded pair tools/gen_golden_group_delay.py feeds to the reference's get_group_delay
  * measure_np           the flow band by band: scipy's zero-phase Butterworth and xcorr_inputs.oracle_delay
  * bounds               azimuth_inputs.flow_bounds' formula with windows of ones and the filter's share as a parameter
  * filter_tolerances    that share per band: filt_inputs.R x scipy's own error against filt_np's compensated blocked statement
  * diag_full            a numpy model of the diagonal scheme of par_find_delay_sect_f64

No device code runs here (filter_tolerances asks the library for its host-side block matrices, like filt_np).
"""
from collections import namedtuple

import numpy as np
import scipy.signal

import azimuth_inputs as A
import filt_inputs as FI
import xcorr_inputs as X

SR, N_FIXTURE, SEED = 44100, 65659, 7
MIN_CORR = 0.6


def fixture_signals(n=N_FIXTURE, sr=SR, seed=SEED):
    """ref: float32 white noise.  src: ref through a first-order Bessel low-pass at 300 Hz, rolled by 7 samples, plus a small
    noise that grows along the file (so that the lowest band, which averages the fewest cycles, correlates worst)."""
    rng = np.random.default_rng(seed)
    ref = rng.standard_normal(n).astype(np.float32)
    sos = scipy.signal.bessel(1, 300, "low", analog=False, output="sos", fs=sr)
    src = np.roll(scipy.signal.sosfilt(sos, ref.astype(np.float64)), 7)
    src = src + 0.02 * np.linspace(0.0, 2.0, n) * rng.standard_normal(n)
    return ref, src.astype(np.float32)


def band_filter(x, lo, hi, sr, order=1):
    """util/filters.py:7-24 restated: band-pass, high-pass, low-pass or the input itself, by which cut-offs lie in (0, Nyquist)"""
    nyq = 0.5 * sr
    low, high = lo / nyq, hi / nyq
    lo_in, hi_in = 0 < low < 1, 0 < high < 1
    if lo_in and hi_in:
        sos = scipy.signal.butter(order, [low, high], btype="band", output="sos")
    elif lo_in:
        sos = scipy.signal.butter(order, low, btype="high", output="sos")
    elif hi_in:
        sos = scipy.signal.butter(order, high, btype="low", output="sos")
    else:
        return np.asarray(x, dtype=np.float64), None
    return scipy.signal.sosfiltfilt(sos, x), np.ascontiguousarray(sos, dtype=np.float64)


Band = namedtuple("Band", "lo hi lag corr level_ref level_src status oracle ya yb sos")


def measure_np(ref, src, sr, edges, order=1, t0=None, t1=None, widen=False):
    """[Band] for every pair of neighbouring edges: experiments/group_delay.py:59-78 in float64.  status 1: the peak sits on the last
    lag (the reference's IndexError); lag and corr are NaN for a row of zeros.
    widen=False hands the signals to scipy in their own dtype, like the reference: sosfiltfilt forms the odd extension of a float32
    signal IN float32 before it filters in float64, which moves a narrow band's correlation by up to 1.1e-9 on the fixture (12-14 Hz);
    group_delay.measure forms the extension the same way.  widen=True converts to float64 first: the flow on float64 input."""
    if widen:
        ref, src = np.asarray(ref, dtype=np.float64), np.asarray(src, dtype=np.float64)
    s_start = 0 if t0 is None else int(t0 * sr)
    s_end = len(src) if t1 is None else int(t1 * sr)
    s_dur = s_end - s_start
    out = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        ya, sos = band_filter(ref[s_start:s_end], float(lo), float(hi), sr, order)
        yb, _ = band_filter(src[s_start:s_end], float(lo), float(hi), sr, order)
        lv = (np.linalg.norm(ya) / np.sqrt(len(ya)), np.linalg.norm(yb) / np.sqrt(len(yb)))
        if not np.any(ya) or not np.any(yb):
            out.append(Band(lo, hi, np.nan, np.nan, lv[0], lv[1], 0, None, ya, yb, sos))
            continue
        try:
            o = X.oracle_delay(ya, yb)
        except IndexError:
            out.append(Band(lo, hi, np.nan, np.nan, lv[0], lv[1], 1, None, ya, yb, sos))
            continue
        out.append(Band(lo, hi, s_dur // 2 - (o.delay + len(ya) // 2), o.corr, lv[0], lv[1], 0, o, ya, yb, sos))
    return out


def bounds(o, nb, eps_a=0.0, eps_b=0.0):
    """azimuth_inputs.flow_bounds' formula: df = SAFETY delta_f(nb) + 2 (eps_a + eps_b) through 3 df / D and
    1.25 df + 0.75 |fm - fp| df / D.  eps: how far the filter may move a NORMALISED row (0 where both sides filter with scipy)."""
    D = abs(o.fm - 2.0 * o.f0 + o.fp)
    df = A.SAFETY * X.delta_f(nb) + 2.0 * (eps_a + eps_b)
    return 3.0 * df / D, 1.25 * df + 0.75 * abs(o.fm - o.fp) * df / D


def odd_ext(x, pad):
    """scipy's extension of sosfiltfilt, in x's own dtype (float32 stays float32), then float64"""
    x = np.asarray(x)
    return np.concatenate((2 * x[:1] - x[pad:0:-1], x, 2 * x[-1:] - x[-2:-pad - 2:-1])).astype(np.float64) if pad else x.astype(np.float64)


def filter_tolerance(sos, x, y_scipy):
    """filt_inputs.R x max(scipy's error against filt_np's compensated blocked statement on this band and signal, FLOOR):
    the existing pin of K_sosfiltfilt, relative to max |y|.  x in the dtype the flow gets it in: both sides filter the same
    extended signal (scipy's extension of a float32 signal is float32's)."""
    import filt_np as FN
    padlen = FI.padlen_of(sos)
    blocked = FN.sosfiltfilt_blocked(sos, scipy.signal.sosfilt_zi(sos), odd_ext(x, padlen), 0, two_level=True)
    return FI.R * max(FI.rel_err(y_scipy, blocked[padlen:len(blocked) - padlen]), FI.FLOOR)


def row_eps(tol, y):
    """flow_bounds' step from a filter tolerance (relative to max |y|) to the move of the normalised row, windows of ones:
    ||e|| <= tol max |y| sqrt(n), and the unit row moves by at most twice that over ||y||"""
    return tol * np.max(np.abs(y)) * np.sqrt(len(y)) / np.linalg.norm(y)


def diag_full(a, b, S):
    """'full' normalised correlation by the diagonal scheme, float64: sections of S samples transformed at N = 2 S, one spectrum
    C_d = sum_{p - q = d} A_p conj(B_q) per offset, full[l] = sum_d c_d[l - d S] over |l - d S| < S.
    -> (full [na + nb - 1], how many diagonals each lag received)"""
    an, bn = X.normalised(a), X.normalised(b)
    na, nb = len(an), len(bn)
    N = 2 * S
    P, Q = -(-na // S), -(-nb // S)
    sect = lambda v, s: np.fft.fft(np.concatenate((v[s * S:(s + 1) * S], np.zeros(N - len(v[s * S:(s + 1) * S])))))
    FA = [sect(an, p) for p in range(P)]
    FB = [sect(bn, q) for q in range(Q)]
    full = np.zeros(na + nb - 1)
    count = np.zeros(na + nb - 1, dtype=np.int64)
    lags = np.arange(-(nb - 1), na)
    for d in range(-(Q - 1), P):
        C = np.zeros(N, dtype=np.complex128)
        for p in range(max(0, d), min(P - 1, d + Q - 1) + 1):
            C += FA[p] * np.conj(FB[p - d])
        c = np.fft.ifft(C).real
        m = lags - d * S
        use = np.abs(m) < S
        full[use] += c[m[use] % N]
        count[use] += 1
    return full, count
