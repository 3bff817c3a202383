"""Float64 / math.fsum statements of the stereo balance tool (pyaudiorestoration_amd/pypan.py, csrc/pan.hip, k_stft_pan in
csrc/stft.hip), the input the fixture tests/golden/pypan.npz was computed from, and the three bounds the tests use.

The measured quantity is fac = mean of q over the cells of a box, q = float32(L / R) for two float32 magnitudes, NaN cells skipped
(np.nanmean).  All three bounds are on fac.

B_ratio (par_pan_ratio_f32 against math.fsum of the float32 quotients formed by numpy from the SAME magnitudes).  The quotients are
equal bit for bit (one correctly rounded float32 division), the count is exact, and math.fsum is the exact sum rounded once.  The
only freedom is the order of a float64 sum of cnt terms: any order is within (cnt - 1) 2^-53 sum|q| of the exact sum, and the
division by cnt adds one rounding, so

    B_ratio = cnt * 2^-52 * mean|q|

(mean over the counted cells; an infinite cell makes sum and bound infinite: such boxes are compared exactly, inf == inf).

B_fused (par_stft_pan_ratio_f32 against par_pan_ratio_f32 on par_stft_f32 mode-1 output).  The fused kernel repeats mode 1's
operations one by one; its float32 magnitudes were found equal to mode 1's bit for bit on the MI355X (NOTES.md, "Stereo balance
(pypan)"), so the quotients are the same set and only the order of the float64 sum differs -- on both sides, each within half
of the figure above of the exact sum: the same bound, B_fused = B_ratio, with the same count.

B_ref (pypan.pan_samples against the fixture's fac, which the reference computed with ITS transform).  Two terms.
  transform   Per frame, a float32 transform's magnitudes are within E = e * max_k |X_frame| of the float64 transform's, with
              e = R_REG * yardstick(M) for the kernel (tests/stft_np.py: the bound test_stft_kernels_gpu.py holds K_stft to, R_REG
              = 8) and e = yardstick(M) for the reference's float32 backend (what yardstick measures; a float64 backend is
              closer still), plus MAG_ULP of the value for the kernel's magnitude step.  For a cell with float64 magnitudes L, R
              and frame peaks PL, PR the two quotients therefore differ by at most
                  dq = q * ((R_REG + 1) * yardstick(M) * (PL / L + PR / R) + 2 * MAG_ULP + 2^-22)
              to first order (2^-22: two float32 divisions).  A cell where the first-order factor exceeds 1/4 is outside the
              linear range; the fixture's boxes hold none (test_pan_cpu checks it), so the term is the mean of dq over the box.
  summation   The reference sums float32 quotients with numpy's pairwise float32 sum.  Measured on the CPU, on the fixture alone:
              S0 = |fixture fac - fsum(fixture's stored cells) / cnt| / fac for the small box (cnt0 cells).  For a box of cnt
              cells the term is 4 * S0 * ceil(log2 cnt) / ceil(log2 cnt0) * fac (pairwise summation grows with the depth of the
              tree; margin 4).  Measured when the fixture was made: S0 = 0 (S0_MEASURED below, NOTES.md carries it too) -- with
              the installed numpy the reference's chain ends in its numpy backend, whose spectra come out float64 (the fixture
              records the dtype), so its quotients and their pairwise sum are float64 and the mean of 95 cells equals fsum's.
              The floor 2^-24 (one float32 rounding of a mean, what a float32 backend could not go below) stands in for 0.
B_ref is measured against the reference and float64 statements only, never against the code under test."""
import math

import numpy as np

import inputs
import stft_np

SEED = 20260
SR = 22050
N = 3 * SR
FFT_SIZE, FFT_OVERLAP = 1024, 4
S0_MEASURED = 0.0               # |fac - fsum / cnt| / fac of the fixture's small box (95 cells), tools/gen_golden_pypan.py prints it
S0_FLOOR = 2.0 ** -24


def stereo_tape(seed=SEED, n=N, sr=SR):
    """(n, 2) float32: one programme (noise under a slow envelope, three tones) with a different slowly varying gain per channel,
    plus independent noise per channel -- a tape whose balance drifts."""
    t = np.arange(n) / sr
    prog = 0.2 * inputs.noise(n, seed) * (0.6 + 0.4 * np.sin(2 * np.pi * 0.7 * t)) + inputs.sine(n, 440.0, sr, 0.1) \
        + inputs.sine(n, 1760.0, sr, 0.05) + inputs.sine(n, 5200.0, sr, 0.03)
    g_l = 1.0 + 0.15 * np.sin(2 * np.pi * 0.21 * t)
    g_r = 0.8 - 0.2 * np.cos(2 * np.pi * 0.13 * t + 0.4)
    out = np.empty((n, 2), dtype=np.float32)
    out[:, 0] = (prog * g_l + 0.004 * inputs.noise(n, seed + 1)).astype(np.float32)
    out[:, 1] = (prog * g_r + 0.004 * inputs.noise(n, seed + 2)).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------ statements
def quotients(L, R):
    """float32(L / R) of two float32 arrays, as numpy divides them"""
    with np.errstate(all="ignore"):
        return np.asarray(L, dtype=np.float32) / np.asarray(R, dtype=np.float32)


def fsum_mean(q):
    """(nanmean of q with the exact sum rounded once, count, mean |q|) -- q any shape; NaN for no cell"""
    v = np.asarray(q, dtype=np.float64).ravel()
    v = v[~np.isnan(v)]
    if v.size == 0:
        return math.nan, 0, math.nan
    if np.any(np.isinf(v)):
        with np.errstate(invalid="ignore"):
            s = float(np.sum(v))                 # +-inf, or NaN for inf - inf, as any order gives
        return s / v.size, int(v.size), math.inf
    return math.fsum(v) / v.size, int(v.size), math.fsum(np.abs(v)) / v.size


def box_fsum(L, R, cell):
    """fsum_mean of box cell = (bin_l, bin_u, frame_0, frame_1) on FRAME-MAJOR magnitudes L, R [frames][>= bins]"""
    bl, bu, f0, f1 = cell
    return fsum_mean(quotients(L[f0:f1, bl:bu], R[f0:f1, bl:bu]))


def b_ratio(cnt, mean_abs):
    return cnt * 2.0 ** -52 * mean_abs


b_fused = b_ratio


def interp_apply(sig, xp, fp):
    """run_resample's product as the FLOAT file stores it"""
    with np.errstate(all="ignore"):
        return (np.asarray(sig) * np.interp(np.arange(len(sig)), xp, fp)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ B_ref
def mags64(x, n_fft, hop, zeropad, frames, win="blackmanharris"):
    """float64 magnitudes [len(frames)][bins] of the float32 frames (stft_np.stft64's statement) for the frames asked"""
    w = stft_np.window32(win, n_fft)
    x = np.asarray(x, dtype=np.float32)
    frames = np.asarray(frames, dtype=np.int64)
    q = frames[:, None] * hop - n_fft // 2 + np.arange(n_fft, dtype=np.int64)[None, :]
    fr = np.zeros((len(frames), n_fft * zeropad), dtype=np.float32)
    fr[:, :n_fft] = w[None, :] * x[stft_np.reflect_idx(q, len(x))]
    return np.abs(np.fft.rfft(fr.astype(np.float64), axis=1)) / math.sqrt(float(n_fft)) + 1e-7


def transform_term(sig, ch_l, ch_r, n_fft, hop, zeropad, cell, r=stft_np.R_REG):
    """-> (B_ref's transform term for the box, the largest first-order factor met in it); r: the kernel's R of stft_np (R_REG for
    the register transform, R_FOUR for the four-step one above 16384 points)"""
    bl, bu, f0, f1 = cell
    if bu <= bl or f1 <= f0:
        return 0.0, 0.0
    frames = np.arange(f0, f1)
    L = mags64(sig[:, ch_l], n_fft, hop, zeropad, frames)
    R = mags64(sig[:, ch_r], n_fft, hop, zeropad, frames)
    e = (r + 1.0) * stft_np.yardstick(n_fft * zeropad)
    pl, pr = L.max(axis=1, keepdims=True), R.max(axis=1, keepdims=True)
    Lb, Rb = L[:, bl:bu], R[:, bl:bu]
    factor = e * (pl / Lb + pr / Rb) + 2 * stft_np.MAG_ULP + 2.0 ** -22
    return float(np.mean(Lb / Rb * factor)), float(factor.max())


def summation_term(fac, cnt, s0, cnt0):
    depth = max(1, math.ceil(math.log2(max(cnt, 2)))) / max(1, math.ceil(math.log2(max(cnt0, 2))))
    return 4.0 * max(s0, S0_FLOOR) * depth * abs(fac)


def b_ref(sig, ch_l, ch_r, n_fft, hop, zeropad, cell, fac, s0, cnt0, r=stft_np.R_REG):
    bl, bu, f0, f1 = cell
    t, _ = transform_term(sig, ch_l, ch_r, n_fft, hop, zeropad, cell, r)
    return t + summation_term(fac, max(0, bu - bl) * max(0, f1 - f0), s0, cnt0)
