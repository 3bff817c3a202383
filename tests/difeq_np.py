"""Shared inputs and oracles of the Differential EQ tests (tests/test_difeq_cpu.py, test_stft_mean_gpu.py, test_difeq_gpu.py).
numpy only.

Kernel oracle (par_stft_mean_db_f32).  The statement in include/par_hip.h: mean[c][b] = (sum over frames f of
20 log10((double) m_f[b])) / n_frames on the float32 magnitudes m_f par_stft_f32 mode 1 writes for the same call.  `mean_db_oracle`
takes those magnitudes and sums every bin with math.fsum (as tests/expander_np.frame_sum_np does), so the only things between it
and the kernel are the kernel's float64 additions, its logarithm and the final division:

    bound[b] = (n_frames + 4) * 2^-53 * sum_f |t_f[b]| / n_frames + 20e-15

n_frames - 1 additions in ANY order lose at most (n_frames - 1) u sum|t| to first order (the run length does not enter), the four
spare u cover the product 20 * log10, the division and second-order terms, and 20e-15 is db_math.h's stated 1e-15 on log10 times
20, which the mean of n_frames such terms cannot exceed.  The bound is about seven orders below what one float32 slip in one
magnitude moves the mean by (2^-24 of a magnitude is 5e-7 dB in that term)."""
import collections
import math
import os

import numpy as np

U = 2.0 ** -53
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MIN_RUN, MAX_RUNS = 16, 512            # include/par_hip.h: R = max(16, ceil(n_frames / 512))


def run_len(n_frames):
    return max(MIN_RUN, -(-n_frames // MAX_RUNS))


def n_frames_of(n, n_fft, hop):
    return (n + 2 * (n_fft // 2) - n_fft) // hop + 1


def scratch_bytes(n, n_fft, hop, zeropad, n_ch):
    nf = n_frames_of(n, n_fft, hop)
    return n_ch * -(-nf // run_len(nf)) * (n_fft * zeropad // 2 + 1) * 8


def mean_db_oracle(mag):
    """mag (frames, bins) float32, all positive and finite -> (mean (bins,), bound (bins,))"""
    mag = np.asarray(mag)
    assert mag.dtype == np.float32 and mag.ndim == 2 and np.all(np.isfinite(mag)) and np.all(mag > 0)
    t = 20.0 * np.log10(mag.astype(np.float64))
    nf, bins = t.shape
    ref, bound = np.empty(bins), np.empty(bins)
    for b in range(bins):
        col = t[:, b].tolist()
        ref[b] = math.fsum(col) / nf
        bound[b] = (nf + 4) * U * math.fsum(abs(v) for v in col) / nf + 20e-15
    return ref, bound


# ------------------------------------------------------------------------------------------------ kernel cases
# sig: zero | imp<position> | loudquiet | noise (tests/stft_np.signal); stride > n_ch leaves channels of NaN between the samples
KCase = collections.namedtuple("KCase", "n_fft zp hop n n_ch stride sig")


def n_for(frames, hop):
    """a signal length with exactly `frames` frames (n_frames = n // hop + 1)"""
    return max(1, hop * (frames - 1) + (1 if hop > 1 else 0))


def kernel_cases():
    c = []
    # every lane geometry: T = 1 lane, below a wave, one wave, two waves (two frames per workgroup), 256 lanes, 1024 lanes;
    # frame counts 1, a run minus / equal / plus one frame, and 2.5 runs (three slots: the last workgroup partly empty wherever it
    # holds more than one slot)
    for M, counts in ((16, (1, 15, 16, 17, 40)), (512, (1, 15, 16, 17, 40)), (1024, (1, 16, 17, 40)), (2048, (1, 15, 17, 40)),
                      (4096, (1, 16, 17, 40)), (16384, (1, 15, 16, 17, 40))):
        for nf in counts:
            hop = M // 2
            c.append(KCase(M, 1, hop, n_for(nf, hop), 1, 1, "noise"))
    # the lane counts between those (T = 2, 8, 16, 512) at hop n_fft / 4: one frame more than the frame slots of a workgroup
    for M, slots in ((32, 128), (128, 32), (256, 16), (8192, 1)):
        c.append(KCase(M, 1, M // 4, n_for(slots + 1, M // 4), 1, 1, "noise"))
    # more than one workgroup at every slot count, a run longer than 16 (n_frames > 8192 -> 17), hop 1
    c += [KCase(16, 1, 1, 4100, 1, 1, "noise"), KCase(16, 1, 1, 8300, 2, 2, "noise"), KCase(512, 1, 256, n_for(147, 256), 2, 2, "noise"),
          KCase(1024, 1, 512, n_for(100, 512), 1, 2, "noise"), KCase(2048, 1, 1024, n_for(70, 1024), 2, 3, "noise")]
    # zero padding 2 and 4 (the frame's tail is zeros; 4096 x 4 is the GUI's largest register-path size)
    c += [KCase(8, 2, 4, 200, 1, 1, "noise"), KCase(4, 4, 2, 77, 2, 2, "noise"), KCase(256, 2, 128, n_for(40, 128), 2, 3, "noise"),
          KCase(512, 2, 256, n_for(33, 256), 1, 1, "noise"), KCase(512, 4, 171, 9000, 2, 2, "noise"),
          KCase(1024, 4, 512, n_for(18, 512), 1, 2, "noise"), KCase(4096, 4, 2048, n_for(20, 2048), 2, 2, "noise"),
          KCase(8192, 2, 4096, n_for(17, 4096), 1, 1, "noise")]
    # an odd hop and a hop above n_fft
    for M in (16, 512, 2048, 16384):
        c.append(KCase(M, 1, (M // 3) | 1, 12 * M + 5, 2, 2, "noise"))
        c.append(KCase(M, 1, M + 3, 19 * (M + 3) + 1, 1, 2, "noise"))
    # signals shorter than n_fft / 2: the reflection folds more than once
    for M in (16, 512, 4096, 16384):
        c += [KCase(M, 1, M // 2, 3, 2, 3, "noise"), KCase(M, 1, M // 4, M // 4 + 1, 1, 1, "noise")]
    # channels and strides on one size per barrier form, and the three special signals
    for M in (512, 2048, 16384):
        hop = M // 2
        n = n_for(21, hop)
        c += [KCase(M, 1, hop, n, 1, 2, "noise"), KCase(M, 1, hop, n, 1, 3, "noise"), KCase(M, 1, hop, n, 2, 2, "noise"),
              KCase(M, 1, hop, n, 2, 3, "noise"), KCase(M, 1, hop, n, 2, 2, "zero"), KCase(M, 1, hop, n, 1, 1, "zero"),
              KCase(M, 1, hop, n, 2, 2, "imp%d" % (3 * hop + 1)), KCase(M, 1, hop, n, 1, 1, "imp0"), KCase(M, 1, hop, n, 2, 3, "loudquiet"),
              KCase(M, 1, hop, n, 1, 1, "loudquiet")]
    return c


def case_id(k):
    return f"{k.n_fft}x{k.zp}-hop{k.hop}-n{k.n}-ch{k.n_ch}of{k.stride}-{k.sig}"


# ------------------------------------------------------------------------------------------------ fixture
PARAM_ORDER = ("highpass", "rolloff_start", "rolloff_end", "resolution", "smoothing", "strength", "keep_gain")


def fixture():
    return np.load(os.path.join(GOLDEN, "difeq.npz"))


def curve_params(g, setting):
    """eq_curve's keyword arguments as the fixture stores them beside the setting's results"""
    p = {k: int(v) for k, v in zip(PARAM_ORDER, g[f"{setting}_params"])}
    p["keep_gain"] = bool(p["keep_gain"])
    return p


def pair_eq(g, pair):
    """get_eq's (rows, bins) result of a stored pair: one stored row stands for all rows of a mono pair"""
    eq = g[f"{pair}_eq"]
    return np.broadcast_to(eq, (int(g[f"{pair}_rows"]), eq.shape[1])) if eq.shape[0] == 1 else eq


def pair_top(g, pair):
    """bins within 60 dB of the peak of BOTH averaged spectra, per row"""
    s, r = g[f"{pair}_src"], g[f"{pair}_ref"]
    top = (s >= s.max(axis=1, keepdims=True) - 60) & (r >= r.max(axis=1, keepdims=True) - 60)
    return np.broadcast_to(top, (int(g[f"{pair}_rows"]), top.shape[1])) if top.shape[0] == 1 else top
