"""Closed-form material for the harmonic / percussive separation fixtures (tools/gen_golden_hpss.py) and tests: steady tones
(harmonic), decaying noise bursts (percussive) and a stretch of exact digital silence longer than the widest median window, so
that the soft mask's "both medians below the smallest normal float" branch is taken."""
import numpy as np

SR = 44100
SECONDS = 1.6
SILENCE = (0.55, 1.05)          # seconds: exact zeros; 0.5 s = 172 hops of 128 samples, above the 99 frames of the widest kernel
TONES = ((330.0, 0.20, 0.3), (1245.0, 0.11, 1.1), (3520.0, 0.07, 2.3), (9100.0, 0.03, 0.5))     # Hz, amplitude, phase
BURSTS = (0.08, 0.21, 0.37, 0.50, 1.12, 1.30, 1.47)                                             # seconds
BURST_DECAY = 0.012             # seconds (time constant)


def tones_bursts_silence(seed=109, sr=SR, seconds=SECONDS):
    """(n,) float32"""
    rng = np.random.default_rng(seed)
    n = int(sr * seconds)
    t = np.arange(n) / sr
    x = sum(a * np.sin(2 * np.pi * f * t + p) for f, a, p in TONES)
    noise = rng.standard_normal(n)
    for t0 in BURSTS:
        x = x + 0.4 * noise * np.where(t >= t0, np.exp(-(t - t0) / BURST_DECAY), 0.0)
    x = x.astype(np.float32)
    x[int(SILENCE[0] * sr):int(SILENCE[1] * sr)] = 0.0
    return x
