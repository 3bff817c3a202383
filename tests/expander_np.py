"""Seeded inputs, float64 numpy oracles and error bounds of the K_expand kernel tests (test_expander_kernels_cpu.py,
test_expander_kernels_gpu.py): the seven entry points of csrc/expander.hip, each against a plain restatement of the operation it
stands for, with math.fsum (or exact integers) where a sum matters.  No torch, no GPU.

Every bound below is derived from the kernel's documented operation order and the number formats, never from what the kernel gives:

frame sums      a lane adds every 4th frame in order (at most ceil(F / 4) - 1 roundings after the first term), three more join
                the lanes, one adds acc: a term passes through at most F / 4 + 4 roundings of 2^-53 each, so
                |got - fsum| <= (F / 4 + 4) 2^-53 (|acc0| + sum |t|); the dB form adds F x 20e-15, log10_pos's documented 1e-15
                against numpy's log10.
window mean     Neumaier's compensated sum returns the exact sum rounded once plus second-order terms (below 1e-6 of the
                first-order one at these lengths), value() rounds once more, the division once: 3 of the 4 x 2^-53 x mean |x|.
expander gain   device pow within 2 ulp, then slope, product and sum of the interpolation each round a value no larger than the
                larger neighbouring factor, then the product with the sample: 8 x 2^-52 x max(fac_j, fac_j+1) x |s|."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
_cache = {}


def _memo(key, make):
    if key not in _cache:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


# ------------------------------------------------------------------------------------------ frame sums (dB and magnitude)
MEAN_BINS = (1, 63, 64, 65, 257)                    # k_mean_db_frames: 64 bins per workgroup
MEAN_FRAMES = (0, 1, 3, 4, 5, 1001)                 # 4 frame lanes
MEAN_PAD = 7                                        # pitch = bins + 7
MAG_SENTINEL = np.float32(3e38)


def mean_case(bins, frames):
    """-> mag (2 * frames, bins) float32 in 1e-6 .. 1e-1 (two chunks of `frames`), acc0 (bins,) float64, nonzero"""
    def make():
        rng = np.random.default_rng(bins * 10007 + frames)
        mag = (10 ** rng.uniform(-6, -1, (2 * frames, bins))).astype(np.float32)
        acc0 = rng.standard_normal(bins) * 10 + np.where(rng.random(bins) < .5, 50.0, -50.0)
        return mag, acc0
    return _memo(("mean", bins, frames), make)


def frame_terms(mag, db):
    m = np.asarray(mag).astype(np.float64)
    if not db:
        return m
    with np.errstate(divide="ignore", invalid="ignore"):
        return 20 * np.log10(m)


def frame_sum_np(mag, acc0, db):
    """-> (acc0[b] + sum_f t[f, b] by fsum, the bound of this call) per bin"""
    t = frame_terms(mag, db)
    frames, bins = t.shape
    ref, bound = np.empty(bins), np.empty(bins)
    for b in range(bins):
        col = t[:, b]
        if np.isfinite(col).all():
            ref[b] = math.fsum([float(acc0[b])] + col.tolist())
        else:
            with np.errstate(invalid="ignore"):
                ref[b] = acc0[b] + np.sum(col)                      # -inf or NaN: no rounding to speak of
        bound[b] = (frames / 4 + 4) * U * math.fsum([abs(float(acc0[b]))] + np.abs(col).tolist()) if np.isfinite(col).all() else 0.0
    if db:
        bound = bound + frames * 20e-15
    return ref, bound


# ------------------------------------------------------------------------------------------ uniform filter, mode "nearest"
UF_ROWS = 3
UF_N = (1, 2, 255, 256, 257, 1000, 20001)
UF_SEG = 256                                        # expander.hip: a thread owns max(size, 256) outputs and slides over them


def uf_sizes(n):
    return tuple(s for s in (1, 3, 255, 257, 513, 2 * n + 1) if s % 2 == 1)


def uf_case(n):
    """(3, n) float64.  Row 0: +-1e8 alternating plus N(0, 1) -- a window sum cancels to the size of one element.  Row 1: N(0, 1)
    with a +-1e8 sample every 97: once it has left the window, a plain running sum keeps its rounding error (1e-8) against a sum of
    the order of 1.  Row 2: 100 + N(0, 1), well conditioned."""
    def make():
        rng = np.random.default_rng(7000 + n)
        x = rng.standard_normal((UF_ROWS, n))
        x[0] += 1e8 * (1 - 2 * (np.arange(n) % 2))
        k = np.arange(40 % n, n, 97)
        x[1, k] = 1e8 * rng.uniform(.5, 1.5, len(k)) * rng.choice([-1.0, 1.0], len(k))
        x[2] += 100.0
        return x
    return _memo(("uf", n), make)


def _exact_ints(row):
    """the float64 values as integers over one common power-of-two denominator"""
    ratios = [float(v).as_integer_ratio() for v in row]
    den = max(d for _, d in ratios)
    return [p * (den // d) for p, d in ratios], den


def uniform_nearest_np(x, size):
    """scipy.ndimage.uniform_filter1d(x, size, mode="nearest") along rows, every window mean exact and rounded once: the window
    sums are differences of an exact integer prefix sum (what math.fsum returns before its rounding), the edge values repeated
    as often as the window overhangs, and Python's integer division rounds the quotient correctly."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    rows, n = x.shape
    h = size // 2
    out = np.empty_like(x)
    for r in range(rows):
        ints, den = _exact_ints(x[r])
        pre = [0] * (n + 1)
        for i, v in enumerate(ints):
            pre[i + 1] = pre[i] + v
        d = den * size
        for i in range(n):
            lo, hi = i - h, i + h
            s = pre[min(hi, n - 1) + 1] - pre[max(lo, 0)] + max(0, -lo) * ints[0] + max(0, hi - (n - 1)) * ints[-1]
            out[r, i] = s / d
    return out


def uniform_nearest_fsum(x, size):
    """the same by math.fsum of every window (the definition; quadratic, for the small shapes of the CPU check)"""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    rows, n = x.shape
    h = size // 2
    idx = np.clip(np.arange(-h, h + 1)[None, :] + np.arange(n)[:, None], 0, n - 1)
    return np.array([[math.fsum(x[r, idx[i]].tolist()) / size for i in range(n)] for r in range(rows)])


def uniform_bound(x, size):
    """4 x 2^-53 x (window mean of |x|), the same windows"""
    return 4 * U * uniform_nearest_np(np.abs(x), size)


def uniform_running_sum(x, size, seg=None):
    """What a plain float64 running sum gives on the kernel's own schedule: segments of max(size, 256) outputs, the first window
    summed directly, then one sample in and one out per output."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    rows, n = x.shape
    h = size // 2
    seg = seg or max(size, UF_SEG)
    out = np.empty_like(x)
    for r in range(rows):
        row = x[r].tolist()

        def at(q):
            return row[0 if q < 0 else (n - 1 if q >= n else q)]
        for i0 in range(0, n, seg):
            s = 0.0
            for q in range(i0 - h, i0 + h + 1):
                s += at(q)
            out[r, i0] = s / size
            for i in range(i0 + 1, min(i0 + seg, n)):
                s += at(i + h)
                s -= at(i - h - 1)
                out[r, i] = s / size
    return out


# ------------------------------------------------------------------------------------------ expander gain
CLIP_LO, CLIP_HI = -120.0, -85.0                    # the GUI's defaults
GAIN_SHAPES = ((1, 1500, 1501), (1, 1500, 700), (64, 4097, 65), (64, 10000, 40), (100, 3333, 34), (2048, 5000, 3),
               (4096, 3000, 1))                     # (hop, n, frames); k_expand_gain: 1024 samples per workgroup
GAIN_CHANNELS = (1, 3)                              # strides n_ch + 2


def gain_case(hop, n, frames, n_ch):
    """-> sig (n, n_ch + 2) float32, curve (n_ch, frames) float64: -130 .. -75 dB (both clips crossed), a fifth of the frames
    exactly on either clip, one NaN frame per channel where there are at least 3 frames"""
    def make():
        rng = np.random.default_rng(hop * 7 + n * 3 + frames + n_ch)
        sig = rng.standard_normal((n, n_ch + 2)).astype(np.float32)
        curve = rng.uniform(-130.0, -75.0, (n_ch, frames))
        pick = rng.random((n_ch, frames))
        curve[pick < .1] = CLIP_LO
        curve[pick > .9] = CLIP_HI
        if frames >= 3:
            for c in range(n_ch):
                curve[c, (frames // 2 + 3 * c) % frames] = np.nan
        return sig, curve
    return _memo(("gain", hop, n, frames, n_ch), make)


def gain_factors(curve):
    with np.errstate(invalid="ignore"):
        return 10.0 ** ((CLIP_HI - np.clip(curve, CLIP_LO, CLIP_HI)) / 20)


def expand_gain_np(sig, curve, hop):
    """-> (ref (n_ch, n) float64 = sig x np.interp(i, j hop, fac), bound (n_ch, n))"""
    n_ch, frames = curve.shape
    n = sig.shape[0]
    fac = gain_factors(curve)
    i = np.arange(n)
    j = np.minimum(i // hop, frames - 1)
    j1 = np.minimum(j + 1, frames - 1)
    ref, bound = np.empty((n_ch, n)), np.empty((n_ch, n))
    for c in range(n_ch):
        s = sig[:, c].astype(np.float64)
        ref[c] = s * np.interp(i, np.arange(frames) * hop, fac[c])
        with np.errstate(invalid="ignore"):
            bound[c] = 8 * 2.0 ** -52 * np.fmax(fac[c, j], fac[c, j1]) * np.abs(s)
    return ref, bound


def nan_reach(curve, hop, n):
    """bool (n_ch, n): the samples strictly between the neighbours of a NaN frame (np.interp returns the frame's own value ON a
    frame, so a NaN frame does not reach its neighbours' samples); everything from it on when it is the last frame"""
    n_ch, frames = curve.shape
    out = np.zeros((n_ch, n), dtype=bool)
    for c in range(n_ch):
        for k in np.flatnonzero(np.isnan(curve[c])):
            lo = (k - 1) * hop + 1 if k > 0 else 0
            hi = (k + 1) * hop if k < frames - 1 else n
            out[c, max(lo, 0):min(hi, n)] = True
    return out


# ------------------------------------------------------------------------------------------ sum rows
SUM_N = (1, 255, 257)


def sum_case(n, n_ch):
    """a, b (n_ch, n) float64; the first samples are float32 ties of the float64 sum (to even: down, then up, and negatives)"""
    def make():
        rng = np.random.default_rng(n * 10 + n_ch)
        a = rng.standard_normal((n_ch, n))
        b = rng.standard_normal((n_ch, n)) * 10 ** rng.uniform(-8, 1, (n_ch, n))
        ties = [(1.0, 2.0 ** -24), (1.0 + 2.0 ** -23, 2.0 ** -24), (-1.0, -2.0 ** -24), (-1.0 - 2.0 ** -23, -2.0 ** -24)]
        for k, (s, d) in enumerate(ties[:n]):
            a[:, k], b[:, k] = s, d
        return a, b
    return _memo(("sum", n, n_ch), make)


# ------------------------------------------------------------------------------------------ normalize
NORM_COUNTS = (1, 255, 4096, 4097, 4194305)         # 4097: a second workgroup; 4194305 = 256 x 16 x 1024 + 1: the 1024-block cap
NORM_GRID_SPAN = 1024 * 256                         # samples the capped grid covers before a thread strides
NORM_PEAK = np.float32(-7.5)


def norm_positions(count):
    """index 0, the last index, and (where the count has one) an index only the stride loop reaches"""
    pos = {0, count - 1}
    if count > NORM_GRID_SPAN:
        pos.add(3 * NORM_GRID_SPAN + 12345)
    return sorted(pos)


def norm_case(count, peak_at):
    def make():
        d = np.random.default_rng(count % 1000003).standard_normal(count).astype(np.float32)
        np.clip(d, -6.0, 6.0, out=d)
        d[peak_at] = NORM_PEAK
        return d
    return _memo(("norm", count, peak_at), make)


def normalize_np(d):
    with np.errstate(invalid="ignore", divide="ignore"):
        return (d / np.max(np.abs(d))).astype(np.float32)


def fraction_mean(values):
    """exact mean as a Fraction (for the CPU check of the integer prefix sums)"""
    return sum((Fraction(float(v)) for v in values), Fraction(0)) / len(values)
