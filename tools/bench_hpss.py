"""Harmonic / percussive separation timings (NOTES.md "HPSS").

    python tools/bench_hpss.py [--files a,b] [--reps 5] [--json out.json]

Files, synthetic and built on the device: a = 10 min at 44.1 kHz stereo, b = 60 min at 192 kHz mono, both at 512/128 (the GUI's
default geometry), kernels 31/31 (default) and 99/99 (the widest).  HIP-event intervals of warm calls (median of --reps):

  k_hpss      par_hpss_f32 alone on the spectrogram of every channel (components: 8 B read + 16 B written per bin)
  transforms  K_stft + 2 x K_istft of every channel, the part of separate around the kernel
  separate    hpss.separate_dev, everything (margin 1: no residual)
  torch       the composed baseline on the same GPU: symmetric padding, unfold(...).median(-1) along both axes, the power-2
              soft mask and the two products of every channel, in chunks of --chunk frames.  --torch-frames N times it on the
              first N frames of a channel only and scales to the file (a quick look; the measured share is printed).

The exit status is 1 when k_hpss does not beat the torch baseline at some kernel size on some file.

From the shapes: algorithmic bytes per bin (24), the achieved share of the HBM peak, and the selection's compare-and-count
pairs per bin (31 passes x (k_h + k_p)), two vector instructions each."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyaudiorestoration_amd import _dev, _lib, decompose, fourier, hpss  # noqa: E402

FILES = {"a": (26_460_000, 44100, 2), "b": (691_200_000, 192000, 1)}
FFT, HOP = 512, 128
KERNELS = ((31, 31), (99, 99))
HBM_BPS = 8.0e12           # MI355X HBM3E peak


def timed(fn, reps, dev):
    fn()
    torch.cuda.synchronize(dev)
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize(dev)
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def torch_hpss(S, kh, kp, chunk):
    """S: complex64 (frames, bins) -> (H, P), odd kernels, power 2, margin 1"""
    mag = S.abs()
    hh, hp = kh // 2, kp // 2
    frames, bins = mag.shape
    padded_f = torch.cat([mag[:hh].flip(0), mag, mag[frames - hh:].flip(0)], dim=0)
    H, P = torch.empty_like(S), torch.empty_like(S)
    tiny = torch.finfo(torch.float32).tiny
    for lo in range(0, frames, chunk):
        hi = min(lo + chunk, frames)
        harm = padded_f[lo:hi + 2 * hh].unfold(0, kh, 1).median(-1).values
        m = mag[lo:hi]
        padded_b = torch.cat([m[:, :hp].flip(1), m, m[:, bins - hp:].flip(1)], dim=1)
        perc = padded_b.unfold(1, kp, 1).median(-1).values
        z = torch.maximum(harm, perc)
        bad = z < tiny
        z = torch.where(bad, torch.ones_like(z), z)
        a, b = (harm / z) ** 2, (perc / z) ** 2
        mh = torch.where(bad, torch.full_like(a, 0.5), a / (a + b))
        mp = torch.where(bad, torch.full_like(a, 0.5), b / (a + b))
        H[lo:hi] = S[lo:hi] * mh
        P[lo:hi] = S[lo:hi] * mp
    return H, P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", default="a,b")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=16384, help="frames per chunk of the torch baseline")
    ap.add_argument("--torch-frames", type=int, default=0, help="frames per channel the torch baseline is timed on (0: the whole file)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = 0
    torch.cuda.set_device(dev)
    L = _lib.lib()
    res = {}
    beaten = True
    for name in a.files.split(","):
        n, sr, ch = FILES[name]
        g = torch.Generator(device=f"cuda:{dev}").manual_seed(3)
        x = torch.empty((n, ch), dtype=torch.float32, device=f"cuda:{dev}")
        step = 1 << 24
        for s in range(0, n, step):                                   # a tone under a slow envelope, over noise
            t = torch.arange(s, min(s + step, n), device=f"cuda:{dev}", dtype=torch.float64) / sr
            tone = (0.3 * torch.sin(2 * math.pi * 440.0 * t) * (1 + 0.5 * torch.sin(2 * math.pi * 3.0 * t))).to(torch.float32)
            x[s:s + step] = tone[:, None] + 0.05 * torch.randn((len(t), ch), generator=g, device=f"cuda:{dev}")
        del t, tone
        window_t = fourier.window_dev("blackmanharris", FFT, dev)
        xpad = torch.zeros(n + FFT // 2, dtype=torch.float32, device=f"cuda:{dev}")
        fms = []
        for c in range(ch):                                           # the spectrogram of every channel, (frames, bins)
            xpad[:n] = x[:, c]
            fms.append(fourier.stft_dev(xpad, FFT, HOP, window_t, 1, 0, dev=dev).T)
        frames, bins = fms[0].shape
        r = {"samples": n, "channels": ch, "frames_per_channel": frames, "bins": bins, "bins_total": frames * bins * ch}
        out = [_dev.empty((frames, bins), torch.complex64, dev) for _ in range(2)]

        def transforms():
            for c in range(ch):
                xpad[:n] = x[:, c]
                s = fourier.stft_dev(xpad, FFT, HOP, window_t, 1, 0, dev=dev)
                fourier.istft_dev(s, HOP, window_t, length=n, dev=dev)
                fourier.istft_dev(s, HOP, window_t, length=n, dev=dev)
        med, best = timed(transforms, a.reps, dev)
        r["transforms_ms"] = med
        for kh, kp in KERNELS:
            k = {}
            med, best = timed(lambda: [decompose.hpss_dev(fm, kh, kp, 2.0, 1.0, 1.0, dev=dev, out=out) for fm in fms], a.reps, dev)
            byts = 24.0 * frames * bins * ch
            k["k_hpss_ms"] = med
            k["k_hpss_ms_min"] = best
            k["algorithmic_bytes_per_bin"] = 24
            k["share_hbm_peak"] = byts / (best * 1e-3) / HBM_BPS
            k["count_pairs_per_bin"] = 31 * (kh + kp)
            k["bins_per_s"] = frames * bins * ch / (best * 1e-3)
            med, best = timed(lambda: hpss.separate_dev(x, FFT, HOP, (kh, kp), 2.0, 1.0, None, dev), max(a.reps // 2, 1), dev)
            k["separate_ms"] = med
            sub = min(frames, a.torch_frames) if a.torch_frames > 0 else frames
            subs = [fm[:sub] for fm in fms]
            med, best = timed(lambda: [torch_hpss(fm, kh, kp, a.chunk) for fm in subs], 2, dev)
            k["torch_measured_frames"] = sub
            k["torch_measured_ms"] = best
            k["torch_ms"] = best * frames / sub
            k["k_hpss_speedup_over_torch"] = k["torch_ms"] / k["k_hpss_ms_min"]
            beaten = beaten and k["k_hpss_ms"] < k["torch_ms"]
            r[f"{kh}/{kp}"] = k
            print(json.dumps({name: {f"{kh}/{kp}": k}}), flush=True)
        res[name] = r
        print(json.dumps({name: {q: v for q, v in r.items() if not isinstance(v, dict)}}), flush=True)
        del x, xpad, fms, out
        torch.cuda.empty_cache()
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)
    if not beaten:
        print("k_hpss did not beat the torch baseline everywhere", file=sys.stderr)
    return 0 if beaten else 1


if __name__ == "__main__":
    sys.exit(main())
