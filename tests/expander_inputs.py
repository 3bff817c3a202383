"""Seeded synthetic material for the Spectral Expander fixtures (tools/gen_golden_expander.py) and tests: a stereo "tape" with
programme in 200-3000 Hz and a hiss above 12 kHz whose level sweeps differently on L and R, so that the default 13-17 kHz noise
floor curve crosses both default clip bounds (-120 and -85 dB)."""
import numpy as np
import scipy.signal

SR = 44100
SECONDS = 3.0


def _hiss(rng, n, sr, level_db):
    """white noise high-passed at 12 kHz, scaled sample by sample to level_db (dB re full scale, RMS before the filter)"""
    sos = scipy.signal.butter(8, 12000, btype="high", fs=sr, output="sos")
    w = scipy.signal.sosfilt(sos, rng.standard_normal(n))
    return w * 10 ** (level_db / 20)


def stereo_tape(seed=7, sr=SR, seconds=SECONDS):
    """(n, 2) float32: tones at 220 / 660 / 1400 / 2900 Hz under a slow envelope on both channels, plus hiss sweeping
    -150 -> -55 -> -150 dB on L and -60 -> -150 -> -70 dB on R"""
    rng = np.random.default_rng(seed)
    n = int(sr * seconds)
    t = np.arange(n) / sr
    env = 0.5 + 0.5 * np.sin(2 * np.pi * 0.7 * t) ** 2
    prog = sum(a * np.sin(2 * np.pi * f * t + p) for f, a, p in ((220, .20, .1), (660, .12, .7), (1400, .08, 1.3), (2900, .05, 2.1)))
    u = t / seconds
    lvl_l = -150 + 95 * np.sin(np.pi * u)                  # up to -55 in the middle
    lvl_r = np.interp(u, (0, .45, 1), (-60, -150, -70))
    left = env * prog + _hiss(rng, n, sr, lvl_l)
    right = env * prog * 0.8 + _hiss(rng, n, sr, lvl_r)
    return np.stack([left, right], axis=1).astype(np.float32)

