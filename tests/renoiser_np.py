"""numpy statement of the renoiser's gate, for the tests (our own words for the rule of renoiser_gui.get_mask_fac and the
product X * fac of run_resample): a bin passes when the float32 decibels of its float32 magnitude |X| + 1e-7 exceed the
float64 threshold, every other bin is scaled by float32(10^(gain/20))."""
import numpy as np


def db32(mag):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float32(20) * np.log10(np.asarray(mag, dtype=np.float32))


def passes(spec, final):
    """spec: complex64 (frames, bins); final: float64 (bins,) -> bool (frames, bins)"""
    mag = (np.abs(spec.astype(np.complex64)) + np.float32(1e-7)).astype(np.float32)
    return db32(mag).astype(np.float64) > np.asarray(final, np.float64)[None, :]


def gate(spec, final, gain):
    fac = np.where(passes(spec, final), np.float32(1.0), np.float32(np.power(10, float(gain) / 20))).astype(np.float32)
    return (spec.astype(np.complex64) * fac).astype(np.complex64)


def reach(frames, hop, n_fft, n):
    """output samples [lo, hi) a bin of each listed frame reaches (istft of the zero-extended signal, length n)"""
    half = n_fft // 2
    return [(max(0, f * hop - half), min(n, f * hop + n_fft - half)) for f in frames]
