"""Float64 restatement of the reference's dynamics matcher (experiments/decompressor_cmd.py:26-188), stage by stage, the
exact-sum variants the kernels are measured against, the input builders and the bounds -- shared by tests/test_dynamics_cpu.py
and tests/test_dynamics_gpu.py.

Every bound comes from the kernel's own summation depth k as gamma_k = k u / (1 - k u), u = 2^-53 (Higham, Accuracy and
Stability of Numerical Algorithms, 3.1-3.4: a sum of k + 1 terms in ANY order has a relative error of at most gamma_k of the sum
of the magnitudes).  None is tuned to what the device gives."""
import math
import os

import numpy as np
import scipy.ndimage
import scipy.signal

U = 2.0 ** -53
HOP, SZ, CORR_SZ, SMOOTHING_SEC, LOWER, UPPER, ORDER, FLOOR = 32, 512, 4096, 0.08, 80, 9000, 3, 0.0005
SR = 44100
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decompressor.npz")


def gamma(k):
    return k * U / (1 - k * U)


def n_frames(n, hop):
    return -(-n // hop)


# ------------------------------------------------------------------------------------------------ the restatement
def bandpass_np(x, lower, upper, sr, order=ORDER):
    """util/filters.py:7-24 for cut-offs inside (0, Nyquist): float32 in, float64 out"""
    sos = scipy.signal.butter(order, [lower / (0.5 * sr), upper / (0.5 * sr)], btype="band", output="sos")
    return scipy.signal.sosfiltfilt(sos, x)


def windowed_rms_np(y, hop, sz):
    """decompressor_cmd.py:16-23"""
    return np.asarray([np.sqrt(np.mean(np.square(y[i:i + sz]))) for i in range(0, len(y), hop)])


def log_curve_np(y, hop, sz, floor=FLOOR):
    """:90-96"""
    with np.errstate(all="ignore"):
        return np.log10(np.clip(windowed_rms_np(y, hop, sz), floor, None))


def level_match_np(a, b):
    """:97"""
    return b - np.mean(b) + np.mean(a)


def uniform_reflect_np(x, size):
    """:99-100 (scipy's default mode)"""
    return scipy.ndimage.uniform_filter1d(x, size=size)


def aligned_np(a, corr_sz):
    """:109-143 with do_sync False: pad by edge values, Hann windows at every corr_hop, overlap-add into zeros, cut"""
    corr_hop = corr_sz // 2
    hann = np.hanning(corr_sz)
    padded = np.pad(a, (corr_hop, corr_hop * 2), "edge")
    acc = np.zeros(padded.shape)
    for x in range(corr_hop, len(a), corr_hop):
        acc[x - corr_hop:x + corr_hop] += padded[x - corr_hop:x + corr_hop] * hann
    return acc[corr_hop:-corr_hop * 2]


def fac_np(b, aligned):
    """:161-166"""
    with np.errstate(all="ignore"):
        fac = np.power(10, b) / np.power(10, aligned)
    np.clip(fac, 0, 2, fac)
    np.nan_to_num(fac, copy=False)
    return fac


def interp_np(fac, n, hop):
    """:169"""
    return np.interp(np.arange(n), np.arange(0, n, hop), fac)


def apply_np(src, facs, hop):
    """:169, 182-185: src (n, ch) float32, facs (ch, F) -> float64 (n, ch)"""
    n, ch = src.shape
    fac_interp = np.empty(src.shape)
    for c in range(ch):
        fac_interp[:, c] = interp_np(facs[c], n, hop)
    return src * np.mean(fac_interp, axis=-1, keepdims=True)


def gain_curves_np(src, ref, sr, hop=HOP, sz=SZ, corr_sz=CORR_SZ, smoothing_sec=SMOOTHING_SEC, lower=LOWER, upper=UPPER, stages=None):
    ns = int(sr * smoothing_sec / hop)
    facs = []
    for c in range(src.shape[1]):
        a = log_curve_np(bandpass_np(src[:, c], lower, upper, sr), hop, sz)
        b = log_curve_np(bandpass_np(ref[:, c], lower, upper, sr), hop, sz)
        b = level_match_np(a, b)
        a, b = uniform_reflect_np(a, ns), uniform_reflect_np(b, ns)
        al = aligned_np(a, corr_sz)
        facs.append(fac_np(b, al))
        if stages is not None:
            stages.append(dict(a=a, b=b, aligned=al))
    return np.asarray(facs)


def match_dynamics_np(src, ref, sr, **kw):
    """process() without the files: float64 (n, ch), what the reference hands to sf.write"""
    return apply_np(src, gain_curves_np(src, ref, sr, **kw), kw.get("hop", HOP))


# ------------------------------------------------------------------------------------------------ exact-sum variants
def rms_exact(y, hop, sz):
    """windowed RMS with the squares and their sum in long double (64-bit significand: the sum's own error is 2^-11 u per term)"""
    y = np.asarray(y, dtype=np.longdouble)
    return np.asarray([np.sqrt(np.sum(np.square(y[i:i + sz])) / len(y[i:i + sz])) for i in range(0, len(y), hop)], dtype=np.longdouble)


def log_curve_exact(y, hop, sz, floor=FLOOR):
    """-> (log10 of the clipped exact RMS as float64, the exact RMS as float64)"""
    with np.errstate(all="ignore"):
        r = rms_exact(y, hop, sz)
        return np.log10(np.clip(r, np.longdouble(floor), None)).astype(np.float64), r.astype(np.float64)


def rms_log_bound(value, sz):
    """|device - exact| of a log10 value: the sum of sz rounded squares in any order is within gamma_k, k = sz + 1 (sz - 1
    additions, the squaring, the division by the count), of the exact mean; the square root halves that and adds its own
    rounding and so does the clip's operand (2 u together); d log10 = d rel / ln 10; log10's own rounding is u |value|."""
    return (gamma(sz + 1) / 2 + 2 * U) / math.log(10) + U * np.abs(value)


def near_floor(rms_exact64, sz, floor=FLOOR):
    """frames whose exact RMS lies within the relative bound of the floor: either side of the clip is right"""
    return np.abs(rms_exact64 - floor) <= (gamma(sz + 1) / 2 + 2 * U) * floor


def level_match_exact(a, b):
    ma, mb = math.fsum(a) / len(a), math.fsum(b) / len(b)
    return np.asarray([float(np.longdouble(v) - np.longdouble(mb) + np.longdouble(ma)) for v in b])


LEVEL_LANES = 1024


def level_bound(a, b, value):
    """gamma_k mean|x| per mean with k = the lane's run (ceil(F / 1024) - 1 additions), the tree (10) and the division (1); plus
    2 u |value| for the subtraction and the addition (inputs are level curves: |b - mean b| <= |value|, which the CPU test
    asserts of every input used)"""
    k = -(-len(b) // LEVEL_LANES) + 10
    return gamma(k) * (np.mean(np.abs(a)) + np.mean(np.abs(b))) + 2 * U * np.abs(value)


def reflect_index(q, n):
    """scipy's "reflect" (d c b a | a b c d | d c b a), repeated as often as needed"""
    m = np.mod(q, 2 * n)
    return np.where(m >= n, 2 * n - 1 - m, m)


def uniform_reflect_exact(x, size):
    """-> (exact window means rounded once more by the division, max |x| over each window)"""
    n = len(x)
    out, peak = np.empty(n), np.empty(n)
    ax = np.abs(x)
    for i in range(n):
        idx = reflect_index(np.arange(i - size // 2, i + size - size // 2), n)
        out[i] = math.fsum(x[idx]) / size
        peak[i] = ax[idx].max()
    return out, peak


def box_bound(peak):
    """the nearest-mode kernel's contract (tests/expander_np.py uniform_bound's constant): 4 u of the window's largest magnitude"""
    return 4 * U * peak


FAC_REL = 2.0 ** -47      # 64 u: two device pow calls at the 16-ulp ceiling of OpenCL-class maths libraries (2 x 16 x 2 u) and the division


def fac_exact(b, aligned):
    """10^b / 10^aligned with mpmath at 80 digits, clipped to [0, 2], NaN -> 0; -> (float64 values, True where the clip or the
    NaN replacement decided the value and the comparison is exact)"""
    import mpmath
    out, hard = np.empty(len(b)), np.zeros(len(b), dtype=bool)
    with mpmath.workdps(80):
        for i, (bv, av) in enumerate(zip(b, aligned)):
            if np.isnan(bv) or np.isnan(av):
                out[i], hard[i] = 0.0, True
                continue
            f = mpmath.power(10, mpmath.mpf(float(bv)) - mpmath.mpf(float(av)))
            if f >= 2 * (1 + mpmath.mpf(FAC_REL)):
                out[i], hard[i] = 2.0, True
            else:
                out[i] = min(float(f), 2.0)
    return out, hard


# ------------------------------------------------------------------------------------------------ input builders
def golden_input(g):
    """(src, ref) float32 (n, 2) from the stored int16 array: src channel 0 = x / 32768, channel 1 = a fixed roll of it; ref =
    float32(src * gain), gain piecewise constant and dyadic (exact)"""
    x = g["x_i16"].astype(np.float32) / np.float32(32768.0)
    src = np.stack((x, np.roll(x, int(g["roll"]))), axis=1)
    gain = np.repeat(g["gain_values"].astype(np.float32), int(g["gain_run"]))[:len(x)]
    return src, (src * gain[:, None]).astype(np.float32)


def make_golden_source(n=140001, seed=20):
    """the int16 array of the fixture: noise whose level moves over 60 dB in steps, a tone, and a digital-silent stretch of
    3000 samples (longer than sz = 512: the 0.0005 floor is reached); n % 32 == 1: the last frame has one sample"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    level = np.repeat(10.0 ** (-rng.integers(0, 13, -(-n // 5000)) / 4.0), 5000)[:n]        # 0 .. -60 dB in 5 dB steps
    x = level * (0.25 * rng.standard_normal(n) + 0.2 * np.sin(2 * np.pi * 440.0 / SR * t))
    x[60000:63000] = 0.0
    return np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)


GOLDEN_ROLL = 777
GOLDEN_GAIN_RUN = 7001
GOLDEN_GAIN_VALUES = np.array([1.0, 0.25, 2.0, 0.5, 0.125, 1.0, 4.0, 0.5, 1.0, 0.0625, 2.0, 0.25, 1.0, 0.5, 8.0, 1.0, 0.25, 0.5, 2.0, 1.0, 0.125])


def golden_rows(n, hop=HOP, corr_sz=CORR_SZ):
    """sample indices the fixture stores: the first and last 4096, every 61st, and every 3rd sample of the frames
    [x_last - corr_hop - 64, x_last + 64) around the overlap-add's tail (all of them would pass the fixture's size limit)"""
    F, ch = n_frames(n, hop), corr_sz // 2
    x_last = ch * ((F - 1) // ch)
    lo, hi = max(0, (x_last - ch - 64) * hop), min(n, (x_last + 64) * hop)
    return np.unique(np.concatenate((np.arange(min(4096, n)), np.arange(lo, hi, 3), np.arange(max(0, n - 4096), n), np.arange(0, n, 61))))


def rms_row(n, seed=3):
    """a band-passed-like float64 row for K_wrms: noise with a loud and a quiet half"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) * np.where(np.arange(n) < n // 2, 0.3, 0.003)


def floor_row(n, hop, sz, floor=FLOOR):
    """a row whose frames lie on both sides of the floor: levels 4 x, 1.2 x, 0.8 x and 0.1 x the floor, and a silent stretch
    longer than sz"""
    rng = np.random.default_rng(11)
    seg = max(1, n // 5)
    lv = np.repeat(np.array([4.0, 1.2, 0.0, 0.8, 0.1, 0.1]) * floor, seg)[:n]
    return rng.standard_normal(n) * lv


def level_rows(rows, F, seed=5):
    """(a, b): log-RMS-like curves in [-3.3, -1.5] whose levels differ by about half a decade"""
    rng = np.random.default_rng(seed + F)
    a = -1.5 - 0.6 * rng.random((rows, F))
    b = -2.0 - 1.3 * rng.random((rows, F))
    return a, b


def box_row(n, seed=7):
    rng = np.random.default_rng(seed + n)
    return -2.0 + rng.standard_normal(n)


def fac_rows(F, corr_sz, seed=9):
    """(a, b) for K_dynfac: log curves around -2 with b - a spread over +-1.5 decades, so that 10^b / 10^aligned clips at 2 for
    some frames and not for others; one b is NaN"""
    rng = np.random.default_rng(seed + F + corr_sz)
    a = -2.0 + 0.5 * rng.standard_normal(F)
    b = a + rng.uniform(-1.5, 1.5, F)
    b[F // 3] = np.nan
    return a, b


def apply_case(n, n_ch, hop, seed=13):
    rng = np.random.default_rng(seed + n + n_ch + hop)
    sig = rng.standard_normal((n, n_ch)).astype(np.float32)
    fac = rng.uniform(0.0, 2.0, (n_ch, n_frames(n, hop)))
    fac[:, ::7] = 2.0
    fac[0, ::5] = 0.0
    return sig, fac
