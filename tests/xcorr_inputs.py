"""Seeded inputs and float64 oracles for the tape-sync correlation path (the X2 block of csrc/stft.hip, correlation.py) and
for the two np.interp kernels of csrc/lag.hip.  No device code is imported here: tests/test_xcorr_inputs_cpu.py proves the
preconditions of every builder with the oracles alone, tests/test_xcorr_gpu.py holds the kernels to them.

Conventions (scipy.signal.correlate on the normalised inputs):
    full[j] = sum_t an[t + j - (nb - 1)] bn[t],  j = 0 .. na + nb - 2
    same[j] = full[j + (nb - 1) // 2],           j = 0 .. na - 1
"""
import math
from collections import namedtuple

import numpy as np
import scipy.signal

U = 2.0 ** -53                          # unit roundoff of float64
RIVAL_TOL = 4.0e-6                      # kXcRivalTol of csrc/stft.hip (include/par_hip.h, par_find_delay_f64)
N_MIN, N_MAX = 1 << 13, 1 << 20         # transform sizes of xc_fft_len
SECTION = N_MAX // 2                    # longer signals are correlated in pairs of sections this long


# ---------------------------------------------------------------------------------------------------------- oracles

def normalised(x):
    x = np.asarray(x, dtype=np.float64)
    return x / np.linalg.norm(x)


def same_direct(a, b):
    """normalised 'same' correlation by direct summation (shapes up to about 8 k)"""
    return scipy.signal.correlate(normalised(a), normalised(b), mode="same", method="direct")


def same_fft(a, b):
    """normalised 'same' correlation through scipy's float64 FFT: places the peak of long shapes"""
    return scipy.signal.correlate(normalised(a), normalised(b), mode="same", method="fft")


def full_fft(a, b):
    return scipy.signal.correlate(normalised(a), normalised(b), mode="full", method="fft")


def exact_at(a, b, lags, full=False):
    """the 'same' (or 'full') correlation at a few lags: math.fsum over the products of the normalised inputs"""
    an, bn = normalised(a), normalised(b)
    na, nb = len(an), len(bn)
    out = []
    for j in lags:
        j = int(j)
        sh = j - (nb - 1) + (0 if full else (nb - 1) // 2)
        t0, t1 = max(0, -sh), min(nb, na - sh)
        out.append(math.fsum((an[t0 + sh:t1 + sh] * bn[t0:t1]).tolist()) if t1 > t0 else 0.0)
    return np.array(out)


def delta_f(nb):
    """rounding of a length-nb float64 dot product of normalised inputs, on either side: sum |a b| <= |a| |b| = 1"""
    return 2.0 * nb * U


def delay_bounds(fm, f0, fp, nb):
    """(|d delay|, |d corr|) between two evaluations of parabolic() whose three values differ by at most delta_f(nb):
    first-order propagation through 0.5 (fm - fp) / D, D = fm - 2 f0 + fp, with |xv - peak| <= 1/2."""
    df = delta_f(nb)
    D = abs(fm - 2.0 * f0 + fp)
    return 3.0 * df / D, 1.25 * df + 0.75 * abs(fm - fp) * df / D


Delay = namedtuple("Delay", "delay corr peak fm f0 fp")


def oracle_delay(a, b, ignore_phase=False, near=1e-12):
    """find_delay in float64 with exact values under the parabola.  The peak lag comes from direct summation on small
    shapes and from the float64 FFT on long ones; lags whose value comes within `near` of the top (the FFT's own error is
    ~1e-15) are decided by exact_at, the lowest lag winning a tie like np.argmax.  f[-1] wraps like numpy's; a peak on the
    last lag is the reference's IndexError."""
    na, nb = len(a), len(b)
    res = same_direct(a, b) if na * nb <= (1 << 26) else same_fft(a, b)
    v = np.abs(res) if ignore_phase else res
    close = np.nonzero(v >= v.max() - near)[0]
    peak = int(close[0])
    if len(close) > 1:
        ex = exact_at(a, b, close)
        ex = np.abs(ex) if ignore_phase else ex
        peak = int(close[int(np.argmax(ex))])
    if peak == na - 1:
        raise IndexError(f"index {na} is out of bounds for axis 0 with size {na}")
    fm, f0, fp = exact_at(a, b, [(peak - 1) % na, peak, peak + 1])
    xv = 0.5 * (fm - fp) / (fm - 2.0 * f0 + fp) + peak
    return Delay(xv - na // 2, f0 - 0.25 * (fm - fp) * (xv - peak), peak, fm, f0, fp)


def rivals_of(v, tol=RIVAL_TOL):
    """the listing rule of the peak stage (k_xcb_peak, the one the single and the batched search share) applied to v
    (|same| under ignore_phase): local maxima within tol of the top, more than two lags from it -> (top, rival lags)"""
    v = np.asarray(v)
    top = int(np.argmax(v))
    left = np.concatenate(([-np.inf], v[:-1]))
    right = np.concatenate((v[1:], [-np.inf]))
    idx = np.nonzero((v >= v[top] - tol) & (v >= left) & (v >= right))[0]
    return top, idx[np.abs(idx - top) > 2]


def xc_fft_len(na, nb):
    """restated from csrc/stft.hip"""
    N = N_MIN
    while N < na + nb - 1 and N < N_MAX:
        N <<= 1
    return N


def section_counts(na, nb):
    """(sections of a, sections of b) of the sectioned form; (1, 1) when one transform holds the correlation"""
    if na + nb - 1 <= N_MAX:
        return 1, 1
    return -(-na // SECTION), -(-nb // SECTION)


# ------------------------------------------------------------------------------------------------ edge-lag builders

EDGE_SHAPES = ((1000, 1000), (1000, 999), (1000, 64), (64, 1000))


def edge_peaks(na):
    return (0, 1, 2, na - 3, na - 2)


def edge_case(na, nb, want, seed=0):
    """two spikes on a 1e-3 noise floor whose 'same' correlation peaks on lag `want`"""
    rng = np.random.default_rng([71, na, nb, want, seed])
    a = 1e-3 * rng.standard_normal(na)
    b = 1e-3 * rng.standard_normal(nb)
    ib = nb // 2
    ia = want + (nb - 1) // 2 - (nb - 1) + ib
    assert 0 <= ia < na
    a[ia] += 1.0
    b[ib] += 1.0
    return a, b


# ----------------------------------------------------------------------------------------- repeated-template builder

TEMPLATE, SPACING, FIRST, LOUDER = 300, 450, 4000, 3e-7


def rival_case(K, loud, scale=1.0 + LOUDER, seed=0):
    """K copies of a 300-sample template of Gaussian noise, 450 samples apart, in `a` from sample 4000 on a 1e-9 floor;
    copy `loud` is multiplied by `scale`; `b` holds one template in the middle.  Under the copies `a` holds the template
    alone, so copies of equal loudness tie exactly.  -> (a, b, the 'same' lag of every copy)"""
    rng = np.random.default_rng([72, K, seed])
    n = 8000 + SPACING * K
    T = rng.standard_normal(TEMPLATE)
    a = 1e-9 * rng.standard_normal(n)
    for k in range(K):
        a[FIRST + SPACING * k:FIRST + SPACING * k + TEMPLATE] = T * (scale if k == loud else 1.0)
    b = np.zeros(n)
    ib = n // 2 - TEMPLATE // 2
    b[ib:ib + TEMPLATE] = T
    lags = FIRST + SPACING * np.arange(K) - ib - (n - 1) // 2 + (n - 1)
    return a, b, lags


RIVAL_KS = (2, 32, 64)


def rival_positions(K):
    return (0, K // 2, K - 1)


def sectioned_rival_case(seed=0):
    """the K = 2 case in the sectioned regime: templates of 4000 samples in 2 x 600 000-sample signals, the louder rival
    400 000 lags behind the first copy"""
    rng = np.random.default_rng([73, seed])
    n, m, first, gap = 600_000, 4000, 100_000, 400_000
    T = rng.standard_normal(m)
    a = 1e-9 * rng.standard_normal(n)
    a[first:first + m] = T
    a[first + gap:first + gap + m] = (1.0 + LOUDER) * T
    b = np.zeros(n)
    ib = n // 2 - m // 2
    b[ib:ib + m] = T
    lags = first + gap * np.arange(2) - ib - (n - 1) // 2 + (n - 1)
    return a, b, lags


# --------------------------------------------------------------------------------------------- size-class builders

def size_classes():
    """[(N, 'fit' | 'min', na, nb)]: for every transform size the exact fit na + nb - 1 == N and the smallest member
    na + nb - 1 == N/2 + 1 (7 + 7 - 1 for the first size); nb about 0.8 na"""
    out = []
    for lg in range(13, 21):
        N = 1 << lg
        for kind, total in (("fit", N + 1), ("min", N // 2 + 2)):
            if kind == "min" and lg == 13:
                out.append((N, kind, 7, 7))
                continue
            na = int(round(total / 1.8)) + (lg & 1)
            out.append((N, kind, na, total - na))
    return out


SECTIONED_SHAPES = ((524_289, 524_289), (700_001, 524_289))
KINDS = ("white", "narrow", "tone", "dc")
# the scratch layout of the single call at the ABI: the smallest transform, the smallest member of the next one, the sectioned form
SCRATCH_SHAPES = ((1000, 999), (4097, 4097), SECTIONED_SHAPES[0])


def sectioned_edge_peaks():
    """edge_case peaks for SECTIONED_SHAPES[0]: lag 0 (f[-1] wraps to the last lag) and the last lag but one"""
    return (0, SECTIONED_SHAPES[0][0] - 2)


def signal_pair(kind, na, nb, seed=0):
    """two takes of one source, `b` delayed and with 1 % of its own noise: white noise, a take band-passed to
    1e-4 .. 6e-4 of the sample rate, a pure tone with a non-integer period, noise on a DC offset of 1"""
    rng = np.random.default_rng([74, KINDS.index(kind), na, nb, seed])
    n = max(na, nb) + 64
    if kind == "tone":
        t = np.arange(n)
        src = np.sin(2.0 * np.pi * t / 123.456 + 0.3)
    else:
        src = rng.standard_normal(n)
        if kind == "narrow":
            sos = scipy.signal.butter(2, [2e-4, 1.2e-3], btype="band", output="sos")
            src = scipy.signal.sosfilt(sos, src)
        if kind == "dc":
            src = src + 1.0
    a = src[:na].copy()
    b = 0.9 * src[17:17 + nb] + 0.01 * rng.standard_normal(nb)
    return a, b


# ------------------------------------------------------------------------------------------------ off-by-lag builder

def flat_top_case(n=500_000, sr=192_000.0, band=(5.0, 15.0), delay=1234.4, seed=0):
    """a Hann-windowed take of 64 partials inside `band` (Hz) and the same take `delay` samples later: the correlation
    is so flat around its peak that the float32 transform's top may sit a lag or two beside the exact one"""
    rng = np.random.default_rng([75, seed])
    f = rng.uniform(band[0], band[1], 64)
    ph = rng.uniform(0.0, 2.0 * np.pi, 64)
    amp = rng.uniform(0.5, 1.0, 64)
    t = np.arange(n, dtype=np.float64)
    a, b = np.zeros(n), np.zeros(n)
    for fk, pk, ak in zip(f, ph, amp):
        a += ak * np.cos(2.0 * np.pi * fk * t / sr + pk)
        b += ak * np.cos(2.0 * np.pi * fk * (t - delay) / sr + pk)
    w = scipy.signal.get_window("hann", n)
    return a * w, b * w


# ------------------------------------------------------------------------------------------------- np.interp inputs

def lerp_oracle(pos, sig):
    return np.interp(pos, np.arange(len(sig)), sig.astype(np.float64), left=0, right=0).astype(np.float32)


def lerp_positions(n, lo, count, seed=0):
    """`count` positions in [lo, n - 1]: random ones, exact integers, n - 1, the next double above n - 1, and -- outside
    the signal -- negative ones, -0.0 and NaN"""
    rng = np.random.default_rng([76, n, seed])
    pos = rng.uniform(lo, n - 1, count)
    k = count // 8
    pos[:k] = np.floor(pos[:k])
    pos[k] = n - 1
    pos[k + 1] = np.nextafter(float(n - 1), np.inf)
    pos[k + 2] = -1.5
    pos[k + 3] = -np.nextafter(0.0, 1.0)
    pos[k + 4] = -0.0
    pos[k + 5] = np.nan
    pos[k + 6] = n - 2
    pos[k + 7] = np.nextafter(float(n - 1), 0.0)
    pos[k + 8] = lo
    return pos


def lerp_nonfinite():
    """{name: (float32 signal, positions)}: samples that are not finite, as a float WAV can hold them, read ON them and between
    them -- np.interp returns fp[j] where x == xp[j] and retries from the right knot where the left one gives NaN, so a neighbour that
    is inf or NaN reaches only the outputs strictly inside its two intervals -- and negative zeros read on them"""
    inf, nan = np.inf, np.nan
    return {
        "inf_and_nan": (np.array([1, inf, inf, 2, nan, 3, 4], np.float32),
                        np.array([0.0, -0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 4.5, 5.0, 5.25, 5.5, 5.75, 6.0])),
        "minus_inf": (np.array([-inf, 0, inf, -inf, -inf, 7], np.float32), np.arange(0.0, 5.01, 0.25)),
        "signed_zero": (np.array([-0.0, 1, -0.0, -0.0, 2, 0.0, -3], np.float32), np.arange(0.0, 6.01, 0.5)),
    }


def lag_curves():
    """{name: (lag curve (m, 2) in seconds, sr, len_signal)}"""
    sr = 48000
    rng = np.random.default_rng(77)
    t = np.sort(rng.uniform(0.0, 0.5, 9))
    return {
        "two_points": (np.array([[0.0, 0.001], [0.5, 0.0035]]), sr, 24000),
        "two_points_negative_lag": (np.array([[0.013, -0.002], [0.41, -0.0071]]), sr, 20011),
        "repeated_time": (np.array([[0.0, 0.0], [0.125, 0.001], [0.25, 0.002], [0.25, 0.0031], [0.5, 0.004]]), sr, 24000),
        "cut_at_0": (np.array([[0.0, -0.6], [0.25, -0.61], [0.5, -0.62]]), sr, 24000),
        "crosses_nowhere": (np.stack((t, rng.uniform(0.001, 0.004, 9)), axis=-1), sr, 24000),
        "crosses_midway": (np.stack((np.concatenate(([0.0], t[1:-1], [0.5])), -rng.uniform(0.001, 0.004, 9)), axis=-1), sr, 24000),
        "x_on_knots": (np.stack((np.arange(9) / 16.0, rng.uniform(-0.002, 0.002, 9)), axis=-1), sr, 24000),
    }
