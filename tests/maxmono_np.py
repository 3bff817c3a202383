"""numpy statements of MaxMono (dropouts_gui.MainWindow.process_max_mono, in our own words), for the tests: per STFT bin the
louder of two channels ("max") and the quieter ("min"); on a tie, and where a magnitude is NaN, both take the right channel."""
import numpy as np


def masks(DL, DR):
    """(|DL| > |DR|, |DL| < |DR|) in the arrays' own precision (complex64 -> numpy's float32 np.abs)"""
    with np.errstate(all="ignore"):
        a, b = np.abs(DL), np.abs(DR)
        return a > b, a < b


def select(DL, DR):
    """(D_max, D_min): np.where copies the chosen cell, bits and all"""
    m_max, m_min = masks(DL, DR)
    return np.where(m_max, DL, DR), np.where(m_min, DL, DR)


def max_mono(signal, fft_size, hop, stft, istft):
    """(y_max, y_min, mask_max, mask_min) of an (n, 2) signal through stft(x, n_fft=, step=) -> (bins, frames) and
    istft(S, hop_length=, length=); the masks are (bins, frames) like the spectra."""
    signal = np.asarray(signal)
    assert signal.ndim == 2 and signal.shape[1] == 2, signal.shape
    n = len(signal)
    pad = np.zeros((n + fft_size // 2, 2), dtype=signal.dtype)                # fix_length(signal, n + fft_size // 2, axis=0)
    pad[:n] = signal
    DL, DR = stft(pad[:, 0], n_fft=fft_size, step=hop), stft(pad[:, 1], n_fft=fft_size, step=hop)
    m_max, m_min = masks(DL, DR)
    y_max = istft(np.where(m_max, DL, DR), hop_length=hop, length=n)
    y_min = istft(np.where(m_min, DL, DR), hop_length=hop, length=n)
    return y_max, y_min, m_max, m_min


def unpack_mask(packed, frames, bins):
    """the fixture's packed bits -> bool (frames, bins)"""
    return np.unpackbits(packed)[:frames * bins].reshape(frames, bins).astype(bool)


def median_bin(DL, DR, frame):
    """the bin of `frame` (spectra frame-major) whose |DL - DR| is the median of the frame's"""
    d = np.abs(np.asarray(DL[frame], np.complex128) - np.asarray(DR[frame], np.complex128))
    return int(np.argsort(d)[len(d) // 2])


NEAR = 2.0 ** -21


def near_ties(SL, SR):
    """bool (frames, bins), spectra frame-major: the bins par_maxmono_stft_f32 may decide differently from the composed route
    (include/par_hip.h): the two magnitudes differ by no more than NEAR x (|L[k]| + |L[H-k]| + |R[k]| + |R[H-k]|)"""
    with np.errstate(all="ignore"):
        a, b = np.abs(np.asarray(SL, np.complex128)), np.abs(np.asarray(SR, np.complex128))
        s = a + a[:, ::-1] + b + b[:, ::-1]
        return np.abs(a - b) <= NEAR * s


def unreached(near, hop, n_fft, n):
    """bool (n,): the output samples no frame with a near-tie bin reaches"""
    ok = np.ones(n, bool)
    half = n_fft // 2
    for f in np.flatnonzero(near.any(axis=1)):
        ok[max(0, f * hop - half):min(n, f * hop + n_fft - half)] = False
    return ok
