"""Offset-gauge timings (NOTES.md "Renoiser: the offset gauge"): K_gauge (par_gauge_offset_f32, renoiser.sniff_offset_dev)
against the composed loop the library allowed before it -- per pad one zero-padded copy, fourier.stft_dev, and torch
reductions (band mean per frame, complex standard deviation).

    python tools/bench_gauge.py [--reps 10] [--composed-reps 3] [--json profiles/gauge_bench.json]

Signal: 4 min at 44.1 kHz mono, synthetic (a tone over noise), built on the device and resident in HBM.  Geometries 2048/512
(the GUI's default, overlap 4) and 2048/128 (experiments/renoiser.py, overlap 16).  Times are HIP-event intervals of warm
calls: median, minimum and maximum of the repeats.  From the shapes: K_gauge's algorithmic work is 2 n N real FMAs (one
N-tap complex FIR at every sample), reported as a share of the float32 vector peak; the composed loop's is hop STFTs."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyaudiorestoration_amd import _dev, fourier, renoiser  # noqa: E402

N, SR = 4 * 60 * 44100, 44100
GEOMS = ((2048, 512), (2048, 128))
FP32_FLOPS = 157.3e12      # MI355X vector FP32 peak


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
    return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "reps": reps}


def composed(x, fft, hop, l, u, window_t, dev):
    """The reference's loop on the device with the entry points the library had before K_gauge"""
    n, half = x.numel(), fft // 2
    stds = torch.empty(hop, dtype=torch.float64, device=x.device)
    for i in range(hop):
        xp = torch.zeros(n + i + half, dtype=torch.float32, device=x.device)
        xp[i:i + n] = x
        spec = fourier.stft_dev(xp, fft, hop, window_t, 1, 0, dev=dev)            # (bins, frames)
        tg = spec[l:u].mean(dim=0).to(torch.complex128)
        stds[i] = torch.sqrt(torch.mean(torch.abs(tg - tg.mean()) ** 2))
    return stds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--composed-reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = 0
    torch.cuda.set_device(dev)
    g = torch.Generator(device=f"cuda:{dev}").manual_seed(3)
    t = torch.arange(N, device=f"cuda:{dev}", dtype=torch.float64) / SR
    x = ((0.3 * torch.sin(2 * math.pi * 5000.0 * t)).to(torch.float32)
         + 0.05 * torch.randn(N, generator=g, device=f"cuda:{dev}")).contiguous()
    del t
    res = {"samples": N, "sample_rate": SR}
    for fft, hop in GEOMS:
        l, u = renoiser.gauge_band(SR, fft)
        window_t = fourier.window_dev(renoiser.WINDOW, fft, dev)
        out = _dev.empty(hop, torch.float64, dev)
        r = {"k_gauge": timed(lambda: renoiser.sniff_offset_dev(x, SR, fft, hop, 0, dev=dev, out=out), a.reps, dev)}
        curve = _dev.to_host(out).copy()
        r["composed"] = timed(lambda: composed(x, fft, hop, l, u, window_t, dev), a.composed_reps, dev)
        ref = _dev.to_host(composed(x, fft, hop, l, u, window_t, dev))
        fmas = 2.0 * N * fft
        r["algorithmic_fma"] = fmas
        r["ratio_composed_over_k_gauge"] = r["composed"]["ms_median"] / r["k_gauge"]["ms_median"]
        r["k_gauge_share_fp32_peak"] = 2.0 * fmas / (r["k_gauge"]["ms_min"] * 1e-3) / FP32_FLOPS
        r["optimal_pad"] = int(np.argmax(curve))
        r["curve_max_abs_diff_vs_composed"] = float(np.max(np.abs(curve - ref)))
        r["curve_max"] = float(curve.max())
        res[f"{fft}/{hop}"] = r
        print(json.dumps({f"{fft}/{hop}": r}), flush=True)
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
