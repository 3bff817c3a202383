"""Yardsticks of the zero-crossing flutter kernels (par_crossing_smooth_f64, par_interp_f64), for test_zerocross_cpu.py and the
GPU tests.

* fold / reflect_index: numpy's np.pad(mode="reflect") index in closed form;
* exact_smooth: the smoothing sum with no rounding but the last -- the periods are integers (as float32) and the weights float64,
  so every product is a rational; they are summed exactly (fractions.Fraction over one power-of-two denominator, the numerators
  as Python integers) and rounded once to float64;
* numpy_chain: the reference's own statement (experiments/zerocrossing_wow.py:17-30): np.diff, np.pad, np.convolve, and np.interp
  for the grid.

The bounds, all derived.  u = 2^-53.  Every term period * weight is >= 0 (Hann weights are >= 0, periods > 0), so the exact sum S
is also the sum of the magnitudes.  A float64 sum of `span` rounded products in ANY order of additions has each product carry
one rounding, (1 + d), and pass through at most span - 1 additions, each (1 + d): |computed - S| <= ((1 + u)^span - 1) S <=
(span + 2) u S for span <= 4096 (span u < 2^-41, the quadratic term is far below 2 u S).  exact_smooth itself is S rounded once,
within u S, which the + 2 also covers.  So
    SMOOTH: |smooth - exact_smooth| <= (span + 2) u exact
    FREQ:   freq = (sr / 2) / smooth adds one division and inherits smooth's error once more through 1 / x: (span + 4) u
    against numpy or the golden, which carry the same bound for their own summation order: the sum, 2 (span + 4) u
    GRID:   np.interp is a convex combination of two knots' values plus three roundings of its own (slope, product, sum) on
            values <= max(fp): (2 (span + 4) + 4) u max(fp), absolute"""
import math
import operator
from fractions import Fraction

import numpy as np
from scipy.signal import get_window

U = 2.0 ** -53


def bound_smooth(span):
    return (span + 2) * U


def bound_freq(span):
    return (span + 4) * U


def bound_vs_numpy(span):
    return 2 * (span + 4) * U


def bound_grid(span):
    return (2 * (span + 4) + 4) * U


def fold(q, n):
    """index into an array of n >= 2 values for the (any integer) position q of its reflect extension"""
    per = 2 * (n - 1)
    k = q % per                      # Python's modulo: non-negative
    return per - k if k >= n else k


def reflect_index(n, width):
    """the indices np.pad(arange(n), width, mode="reflect") holds"""
    return np.array([fold(i - width, n) for i in range(n + 2 * width)], dtype=np.int64)


def periods(crossings):
    """np.diff(crossings).astype(np.float32): int64 difference, one rounding"""
    return np.diff(np.asarray(crossings, dtype=np.int64)).astype(np.float32)


def hann_kernel(span):
    return get_window("hann", int(span)) / int(span) * 2


def exact_smooth(d, kernel):
    """smooth[i] = sum_j P[i + span + (span - 1) // 2 - j] * kernel[j] in exact arithmetic, rounded once -> float64 (n,)"""
    n, span = len(d), len(kernel)
    h = (span - 1) // 2
    # Fractions over one denominator: every weight is a whole multiple of 2^(e - 53) (e its binary exponent) and every period a
    # whole number, so the numerators are summed as Python integers (exact) and the Fraction is formed, and rounded, once per output
    one = 1 << max([53 - math.frexp(float(v))[1] for v in kernel if v != 0] + [0])
    dq = [Fraction(float(v)) for v in d]
    assert all(v.denominator == 1 for v in dq)
    di = [v.numerator for v in dq]
    wi = [int(Fraction(float(v)) * one) for v in kernel]
    assert all(Fraction(w, one) == Fraction(float(v)) for w, v in zip(wi, kernel))
    per = 2 * (n - 1)
    taps = np.arange(span)
    out = np.empty(n, dtype=np.float64)
    for i in range(n):
        k = (i + h - taps) % per
        k = np.where(k >= n, per - k, k)
        acc = sum(map(operator.mul, [di[x] for x in k.tolist()], wi))
        out[i] = float(Fraction(acc, one))              # Fraction -> float is correctly rounded
    return out


def numpy_smooth(d, kernel):
    """the reference's lines 25-28 on float32 periods d"""
    span = len(kernel)
    return np.convolve(np.pad(d, span, mode="reflect"), kernel, mode="same")[span:-span]


def numpy_chain(crossings, sr, span, t0=0.0, grid=None):
    """-> dict(d, smooth, freq, xp, raw[, grid_freqs]) as the reference computes them (sr a Python number, as the script's)"""
    crossings = np.asarray(crossings, dtype=np.int64)
    d = periods(crossings)
    smooth = numpy_smooth(d, hann_kernel(span))
    out = {"d": d, "smooth": smooth, "freq": sr / 2 / smooth, "xp": crossings[:len(d)] / sr + t0,
           "raw": (np.float32(sr / 2) / d).astype(np.float32)}
    if grid is not None:
        out["grid_freqs"] = np.interp(grid, out["xp"], out["freq"])
    return out


def pilot(sr, hz, seconds, depth, flutter_hz, noise, seed):
    """float32 pilot tone with sinusoidal flutter of relative depth `depth` and white noise"""
    t = np.arange(int(round(sr * seconds))) / sr
    speed = 1.0 + depth * np.sin(2 * np.pi * flutter_hz * t)
    phase = 2 * np.pi * hz * np.cumsum(speed) / sr
    return (0.5 * np.sin(phase + 0.3) + noise * np.random.default_rng(seed).standard_normal(len(t))).astype(np.float32)
