"""Stereo balance timings (NOTES.md "Stereo balance (pypan)"): measuring 1, 8 and 64 boxes of a 10-minute stereo file by

  fused      par_stft_pan_ratio_f32 (pypan.pan_samples_dev, FUSED on): the boxes' frames of both channels transformed, divided and
             summed in one launch; no spectrogram stored
  composed   par_stft_f32 mode 1 of either channel, whole file, then par_pan_ratio_f32 (pypan.pan_samples_dev, FUSED off)
  torch      torch.stft of either channel, |X| / sqrt(n_fft) + 1e-7, the float32 quotient of the box and its float64 nanmean

and applying the pan line to the right channel (par_pan_apply_f32, pypan.apply_pan_dev).

    python tools/bench_pypan.py [--reps 10] [--json profiles/pypan_bench.json]

Signal: 10 min at 44.1 kHz, two channels interleaved, synthetic (a common programme, a gain per channel, independent noise), built
on the device and resident in HBM.  FFT 4096, overlap 8 (hop 512), Blackman-Harris.  A box is 3 s by 300 .. 5000 Hz (259 frames,
436 bins); the boxes are spread evenly over the file.  Times are HIP-event intervals of warm calls: median, minimum and maximum of
the repeats.  From the shapes: the fused launch's algorithmic traffic is the boxes' samples of both channels read once (frames of
a box overlap 7/8) and 16 bytes written per (box, frame); the composed path's is the file read twice and two magnitude
spectrograms written and, inside the boxes, read."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyaudiorestoration_amd import _dev, fourier, pypan  # noqa: E402

SR, SECONDS = 44100, 600
N = SR * SECONDS
FFT, OVERLAP = 4096, 8
BOX_S, BOX_HZ = 3.0, (300.0, 5000.0)
COUNTS = (1, 8, 64)


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


def boxes_of(count):
    starts = np.linspace(5.0, SECONDS - 5.0 - BOX_S, count)
    return [(float(t), BOX_HZ[0], float(t) + BOX_S, BOX_HZ[1]) for t in starts]


def torch_composition(sig, cells, window_t):
    mags = []
    for c in (0, 1):
        spec = torch.stft(sig[:, c].contiguous(), FFT, hop_length=FFT // OVERLAP, window=window_t, center=True, pad_mode="reflect",
                          return_complex=True)
        mags.append(spec.abs() / math.sqrt(FFT) + 1e-7)                       # (bins, frames) float32
    out = torch.empty(len(cells), dtype=torch.float64, device=sig.device)
    for k, (bl, bu, f0, f1) in enumerate(cells):
        out[k] = torch.nanmean((mags[0][bl:bu, f0:f1] / mags[1][bl:bu, f0:f1]).to(torch.float64))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = 0
    torch.cuda.set_device(dev)
    g = torch.Generator(device=f"cuda:{dev}").manual_seed(5)
    t = torch.arange(N, device=f"cuda:{dev}", dtype=torch.float64) / SR
    prog = (0.2 * torch.sin(2 * math.pi * 440.0 * t) + 0.1 * torch.sin(2 * math.pi * 1760.0 * t)).to(torch.float32) \
        + 0.1 * torch.randn(N, generator=g, device=f"cuda:{dev}")
    sig = torch.empty((N, 2), dtype=torch.float32, device=f"cuda:{dev}")
    sig[:, 0] = prog * (1.0 + 0.15 * torch.sin(2 * math.pi * 0.01 * t)).to(torch.float32) + 0.004 * torch.randn(N, generator=g, device=f"cuda:{dev}")
    sig[:, 1] = prog * (0.8 - 0.2 * torch.cos(2 * math.pi * 0.007 * t)).to(torch.float32) + 0.004 * torch.randn(N, generator=g, device=f"cuda:{dev}")
    del t, prog
    window_t = fourier.window_dev(pypan.WINDOW, FFT, dev)
    hop = FFT // OVERLAP
    res = {"samples": N, "sample_rate": SR, "channels": 2, "fft_size": FFT, "hop": hop, "box_seconds": BOX_S, "box_hz": BOX_HZ}
    for count in COUNTS:
        boxes = boxes_of(count)
        fac, cells = pypan.pan_samples_dev(sig, SR, boxes, FFT, OVERLAP, dev=dev, fused=True)
        fac = _dev.to_host(fac)
        r = {"cells": [int(v) for v in cells[0]], "box_frames": int(sum(c[3] - c[2] for c in cells))}
        r["fused"] = timed(lambda: pypan.pan_samples_dev(sig, SR, boxes, FFT, OVERLAP, dev=dev, fused=True), a.reps, dev)
        r["composed"] = timed(lambda: pypan.pan_samples_dev(sig, SR, boxes, FFT, OVERLAP, dev=dev, fused=False), a.reps, dev)
        r["torch"] = timed(lambda: torch_composition(sig, cells, window_t), a.reps, dev)
        composed = _dev.to_host(pypan.pan_samples_dev(sig, SR, boxes, FFT, OVERLAP, dev=dev, fused=False)[0])
        via_torch = _dev.to_host(torch_composition(sig, cells, window_t))
        r["fused_minus_composed_max_abs"] = float(np.max(np.abs(fac - composed)))
        r["fused_minus_torch_max_rel"] = float(np.max(np.abs(fac - via_torch) / np.abs(fac)))
        r["fused_algorithmic_bytes"] = int(sum(((c[3] - c[2] - 1) * hop + FFT) * 8 + (c[3] - c[2]) * 16 for c in cells))
        r["composed_algorithmic_bytes"] = int(2 * N * 4 + 2 * (N // hop + 1) * (FFT // 2 + 1) * 4
                                              + sum(2 * (c[3] - c[2]) * (c[1] - c[0]) * 4 for c in cells))
        r["ratio_composed_over_fused"] = r["composed"]["ms_median"] / r["fused"]["ms_median"]
        r["ratio_torch_over_fused"] = r["torch"]["ms_median"] / r["fused"]["ms_median"]
        r["fac_first"] = float(fac[0])
        res[f"boxes_{count}"] = r
        print(json.dumps({f"boxes_{count}": r}), flush=True)
    markers = [pypan.PanSample(b[:2], b[2:], float(v)) for b, v in zip(boxes, fac)]
    curve = pypan.pan_line(markers, SECONDS, SR, hop)
    out = _dev.empty(N, torch.float32, dev)
    r = timed(lambda: pypan.apply_pan_dev(sig, SR, curve, 1, dev, out=out), a.reps, dev)
    r["curve_rows"] = int(len(curve))
    r["algorithmic_bytes"] = int(N * 8 + curve.nbytes)
    r["gbytes_per_s_at_min"] = r["algorithmic_bytes"] / (r["ms_min"] * 1e-3) / 1e9
    res["apply"] = r
    print(json.dumps({"apply": r}), flush=True)
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
