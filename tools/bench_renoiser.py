"""Renoiser timings (NOTES.md "Renoiser"): the fused gate (par_gate_stft_f32, one launch for both channels) against the composed
device path (K_stft -> par_gate_spectrum_f32 -> K_istft per channel), device -> device and numpy -> numpy (renoise).

    python tools/bench_renoiser.py [--reps 10] [--json out.json]

File: 10 min at 44.1 kHz stereo, synthetic (a tone over noise), built on the device.  Geometries 2048/512 (the GUI's default),
2048/128 (experiments/renoiser.py) and 16384/4096 (above 8192: composed only).  Device times are HIP-event intervals of warm calls
(median of --reps); kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script.  From the shapes:
algorithmic bytes (fused: 4 B read + 4 B written per channel-sample; composed: + 8 B x bins per frame written and read back, and
the zero-extended copy), real-FFT flops 2 x 2.5 M log2 M per frame (forward and inverse), and the redundant-frame share of the
streaming kernel (par_gate_stft_transformed_frames against the frames the ISTFT needs)."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyaudiorestoration_amd import _dev, _lib, renoiser  # noqa: E402

N, SR, CH = 26_460_000, 44100, 2
GEOMS = ((2048, 512), (2048, 128), (16384, 4096))
HBM_BPS = 8.0e12           # MI355X HBM3E peak
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
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = 0
    torch.cuda.set_device(dev)
    g = torch.Generator(device=f"cuda:{dev}").manual_seed(3)
    t = torch.arange(N, device=f"cuda:{dev}", dtype=torch.float64) / SR
    tone = (0.3 * torch.sin(2 * math.pi * 440.0 * t)).to(torch.float32)
    x = (torch.stack([tone, torch.roll(tone, 4321)], dim=1) + 0.01 * torch.randn((N, CH), generator=g, device=f"cuda:{dev}")).contiguous()
    del t, tone
    x_np = _dev.to_host(x)
    L = _lib.lib()
    res = {"samples": N, "channels": CH}
    for fft, hop in GEOMS:
        prof = renoiser.noise_profile(x[:SR * 5, :1].contiguous(), SR, SR, fft, hop, dev)
        final = renoiser.final_profile(prof, SR, fft)
        out = _dev.empty((N, CH), torch.float32, dev)
        frames = (N + fft // 2) // hop + 1
        bins = fft // 2 + 1
        M = fft
        r = {"frames_per_channel": frames}
        flops = CH * frames * 2 * 2.5 * M * math.log2(M)
        paths = (True, False) if renoiser.fused_supported(fft, hop) else (False,)
        for fused in paths:
            name = "fused" if fused else "composed"
            med, best = timed(lambda: renoiser.renoise_dev(x, final, 12.0, fft, hop, None, dev, fused=fused, out=out), a.reps, dev)
            byts = 8.0 * N * CH if fused else 8.0 * N * CH + CH * (2 * 8.0 * frames * bins + 8.0 * (N + fft // 2))
            r[name] = {"device_ms": med, "device_ms_min": best, "algorithmic_bytes": byts, "fft_flops": flops,
                       "share_hbm_peak": byts / (best * 1e-3) / HBM_BPS, "share_fp32_peak": flops / (best * 1e-3) / FP32_FLOPS}
        if renoiser.fused_supported(fft, hop):
            need = min(frames, -(-(N + fft) // hop))
            done = int(L.par_gate_stft_transformed_frames(N, fft, hop))
            r["redundant_frame_fraction"] = 1.0 - need / done
        renoiser.renoise(x_np, SR, final, 12.0, fft, hop)              # warm
        ts = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            renoiser.renoise(x_np, SR, final, 12.0, fft, hop)
            ts.append(time.perf_counter() - t0)
        r["numpy_to_numpy_s"] = float(np.median(ts))
        res[f"{fft}/{hop}"] = r
        print(json.dumps({f"{fft}/{hop}": r}), flush=True)
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
