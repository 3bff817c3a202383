"""float64 statements of the renoiser's "Gauge offset" (reference renoiser_gui.py:347-369) for the K_gauge tests: the reference's
loop written out literally, its FIR form, a float32 emulation of the kernel's summation order, and the error bound the GPU
tests use as their tolerance (derivation: NOTES.md "Renoiser: the offset gauge")."""
import numpy as np
from scipy import signal as dsp

SR = 44100
BAND = (3000, 12000)
U32 = 2.0 ** -24                      # unit roundoff of float32

# (n_fft, hop, n): the smallest shapes that reach each path of the kernel
GPU_SHAPES = {
    "smallest": (16, 4, 50),
    "small": (64, 8, 1000),
    "hop_is_n_fft": (64, 64, 1500),
    "not_pow2_hop_not_dividing": (50, 7, 333),
    "shorter_than_frame": (256, 32, 100),
    "default_chunks_and_tiles": (2048, 128, 20000),
}
IMPULSE_SHAPE = (64, 8, 203)
TONE_SHAPE = (64, 8, 1000)            # 5512.5 Hz at 44.1 kHz: a period of 8 samples = the hop


def noise(n, seed=0):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32) * np.float32(0.1)


def noise_and_tone(n, seed=1, f=5000.0):
    t = np.arange(n, dtype=np.float64)
    return (noise(n, seed).astype(np.float64) + 0.3 * np.sin(2 * np.pi * f * t / SR)).astype(np.float32)


def tone(n, f=5512.5):
    return (0.5 * np.sin(2 * np.pi * f * np.arange(n, dtype=np.float64) / SR)).astype(np.float32)


def impulse(n, at):
    x = np.zeros(n, dtype=np.float32)
    x[at] = 1.0
    return x


def band_bins(sr, n_fft, band=BAND):
    """renoiser_gui.py:352-353, with the slice's clip"""
    l = int(round(band[0] * n_fft / sr))
    u = int(round(band[1] * n_fft / sr))
    return l, min(u, n_fft // 2 + 1)


def padded(x, i, n_fft):
    """The signal the reference's STFT frames for pad i: np.pad(x, (i, 0)), fix_length to n + i + n_fft // 2, and
    fourier.stft's np.pad(..., n_fft // 2, mode="reflect"), float64."""
    x = np.asarray(x, dtype=np.float64)
    p = np.pad(x, (i, 0))
    p = np.pad(p, (0, len(x) + i + n_fft // 2 - len(p)))
    return np.pad(p, n_fft // 2, mode="reflect")


def frames_of(p, n_fft, hop):
    """(frames, n_fft) view of the padded signal: frame j = p[j hop : j hop + n_fft], (len(p) - n_fft) // hop + 1 of them"""
    return np.lib.stride_tricks.sliding_window_view(p, n_fft)[::hop]


def complex_std(z):
    return float(np.std(np.asarray(z, dtype=np.complex128)))


def reference_stds(x, sr, n_fft, hop, band=BAND):
    """The reference's loop, literally, in float64: for every pad the STFT (float32 blackmanharris window, rfft / sqrt(n_fft)),
    the mean of rows l:u per frame, and the complex std of that series."""
    window = dsp.get_window("blackmanharris", n_fft).astype(np.float32)
    l, u = band_bins(sr, n_fft, band)
    stds = np.empty(hop, dtype=np.float64)
    for i in range(hop):
        p = padded(x, i, n_fft)
        n_est = (len(p) - n_fft) // hop + 1
        spec = np.empty((n_fft // 2 + 1, n_est), dtype=np.complex128)
        for j in range(n_est):
            spec[:, j] = np.fft.rfft(window * p[j * hop: j * hop + n_fft]) / np.sqrt(n_fft)
        time_gain = np.average(spec[l:u, :], axis=0)
        stds[i] = time_gain.std()
    return stds


def fir_stds(x, h, n_fft, hop):
    """The FIR form in float64: z(i, j) = sum_m p_i[j hop + m] h[m]"""
    h = np.asarray(h, dtype=np.complex128)
    return np.array([complex_std(frames_of(padded(x, i, n_fft), n_fft, hop) @ h) for i in range(hop)])


def emulate_f32(x, h32_re, h32_im, n_fft, hop):
    """The kernel's arithmetic: each part of z is one float32 FMA chain over ascending m (float32(acc + p * h) with the product
    and sum in float64: the product of two float32 is exact there, the sum rounds to 53 bits before it rounds to 24, which moves
    a result by at most 2^-53 relative against a true FMA); the moments are float64 and std = sqrt(max(0, S2/F - |S/F|^2))."""
    hr = np.asarray(h32_re, dtype=np.float32).astype(np.float64)
    hi = np.asarray(h32_im, dtype=np.float32).astype(np.float64)
    stds = np.empty(hop, dtype=np.float64)
    per = max(1, 4096 // max(1, (len(x) + n_fft) // hop + 1))          # pads per batch
    for i0 in range(0, hop, per):
        blocks = [frames_of(padded(x, i, n_fft), n_fft, hop) for i in range(i0, min(hop, i0 + per))]
        P = np.ascontiguousarray(np.concatenate(blocks).T)           # (n_fft, rows)
        re = np.zeros(P.shape[1], dtype=np.float32)
        im = np.zeros(P.shape[1], dtype=np.float32)
        for m in range(n_fft):
            re = (re.astype(np.float64) + P[m] * hr[m]).astype(np.float32)
            im = (im.astype(np.float64) + P[m] * hi[m]).astype(np.float32)
        at = 0
        for k, b in enumerate(blocks):
            zr = re[at:at + len(b)].astype(np.float64)
            zi = im[at:at + len(b)].astype(np.float64)
            at += len(b)
            F = len(b)
            var = np.sum(zr * zr + zi * zi) / F - ((np.sum(zr) / F) ** 2 + (np.sum(zi) / F) ** 2)
            stds[i0 + k] = np.sqrt(max(0.0, var))
    return stds


def sum_constant(n_fft):
    """c of the bound: n_fft roundings of the FMA chain with their second-order terms, n_fft u / (1 - n_fft u) = gamma_n;
    + 1 for the rounding of h to float32; + 1 for the float64 moments (below)."""
    return n_fft / (1.0 - n_fft * U32) + 2.0


def bound(x, h32, n_fft, hop):
    """Per pad, the largest distance between the kernel's curve and the float64 one that float32 arithmetic allows:
        max_j c 2^-24 sum_m |p_i[j hop + m]| |h[m]|,      c = sum_constant(n_fft) <= n_fft + 3 (n_fft <= 4096).
    std is a seminorm of the series, so |std(z + d) - std(z)| <= max_j |d_j|; a part's FMA chain over ascending m errs by at most
    gamma_n sum |p| |h_part| (n roundings), the two parts together by at most gamma_n sum |p| |h| (Minkowski); rounding h to
    float32 moves z by at most u sum |p| |h|.  The float64 moments: S and S2 are compensated sums joined by a tree of depth 8, the
    variance takes 6 more operations, so var errs by less than 18 2^-53 mean|z|^2 and std -- at worst, where the variance
    vanishes -- by less than sqrt(18 2^-53) rms|z| = 4.5e-8 rms|z| <= 2^-24 max_j sum |p| |h|: the last unit of c."""
    h_abs = np.abs(np.asarray(h32, dtype=np.complex128))
    c = sum_constant(n_fft)
    return np.array([c * U32 * float(np.max(frames_of(np.abs(padded(x, i, n_fft)), n_fft, hop) @ h_abs)) for i in range(hop)])
