"""Differential EQ timings (NOTES.md "Differential EQ"): the time-averaged dB spectra of a stereo file by

  fused      par_stft_mean_db_f32 (spectrum_flat.mean_spectra_db_dev, fused=True): both channels in one launch, frames summed in
             registers, one partial row per run of frames; no spectrogram stored
  composed   per channel, fourier.stft_dev mode 1 over frame chunks and par_mean_db_frames_f32 (fused=False): the path
             spectrum_flat.spectra_from_audio has always taken, unchanged code

at 16384 / 8192 on 10 min at 44.1 kHz and on 60 min at 192 kHz (difeq's shape) and at 4096 / 256 on 10 min at 44.1 kHz
(spectrum_flat's default shape); and difeq.get_eq file to file (two 10-minute stereo WAV files) with either path.

    python tools/bench_difeq.py [--reps 20] [--json profiles/difeq_bench.json] [--skip-long] [--skip-files]

Protocol: the signal is synthetic noise resident in HBM.  After two warm calls of each path, fused and composed alternate for
`reps` rounds in one process, every call timed by HIP events around it; the medians are reported.  Then the composed path is
repeated alone in three more series of `reps` calls: `spread_ms` is the distance between the largest and the smallest of its four
medians.  `fused_not_slower` is fused median <= composed median + spread.  get_eq is wall-clock time (file reading and decoding,
upload, spectra, download), median of 5 alternating calls.  Algorithmic bytes: fused reads the samples once and writes and reads
the partial rows; composed reads the samples once per channel and writes and reads both magnitude spectrograms."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyaudiorestoration_amd import _lib, difeq, io_ops, spectrum_flat  # noqa: E402

SHAPES = (("difeq_10min_44k", 16384, 8192, 44100, 600), ("difeq_60min_192k", 16384, 8192, 192000, 3600),
          ("default_10min_44k", 4096, 256, 44100, 600))


def noise(n, ch, dev):
    g = torch.Generator(device=f"cuda:{dev}").manual_seed(11)
    sig = torch.empty((n, ch), dtype=torch.float32, device=f"cuda:{dev}")
    step = 1 << 26
    for s in range(0, n, step):
        sig[s:s + step] = 0.1 * torch.randn((min(step, n - s), ch), generator=g, device=f"cuda:{dev}")
    return sig


def once(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def stats(ts):
    return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "reps": len(ts)}


def measure(sig, n_fft, hop, reps, dev):
    fused = lambda: spectrum_flat.mean_spectra_db_dev(sig, n_fft, hop, (0, 1), fused=True, dev=dev)
    composed = lambda: spectrum_flat.mean_spectra_db_dev(sig, n_fft, hop, (0, 1), fused=False, dev=dev)
    for _ in range(2):
        fused(), composed()
    torch.cuda.synchronize(dev)
    tf, tc = [], []
    for _ in range(reps):
        tf.append(once(fused, dev))
        tc.append(once(composed, dev))
    alone = [[once(composed, dev) for _ in range(reps)] for _ in range(3)]
    medians = [float(np.median(tc))] + [float(np.median(s)) for s in alone]
    spread = max(medians) - min(medians)
    a, b = fused().cpu().numpy(), composed().cpu().numpy()
    n, bins = sig.shape[0], n_fft // 2 + 1
    frames = int(_lib.lib().par_stft_frames(n, n_fft, hop))
    scratch = int(_lib.lib().par_stft_mean_db_scratch_bytes(n, n_fft, hop, 1, 2))
    r = {"samples": n, "fft_size": n_fft, "hop": hop, "frames": frames, "fused": stats(tf), "composed": stats(tc),
         "composed_alone_medians_ms": medians[1:], "spread_ms": spread,
         "ratio_composed_over_fused": float(np.median(tc) / np.median(tf)),
         "fused_not_slower": bool(np.median(tf) <= np.median(tc) + spread),
         "fused_minus_composed_max_abs_db": float(np.max(np.abs(a - b))),
         "fused_algorithmic_bytes": int(n * 8 + 2 * scratch + 2 * bins * 8),
         "composed_algorithmic_bytes": int(2 * n * 8 + 2 * 2 * frames * bins * 4 + 2 * bins * 8)}
    return r


def measure_files(reps, dev):
    sr, n = 44100, 44100 * 600
    tmp = tempfile.mkdtemp()
    try:
        paths = []
        for k in range(2):
            sig = (0.1 * np.random.default_rng(k).standard_normal((n, 2))).astype(np.float32)
            paths.append(os.path.join(tmp, f"{k}.wav"))
            io_ops.write_wav_float(paths[-1], sig, sr)
        del sig
        ts = {True: [], False: []}
        for i in range(reps + 1):
            for fused in (True, False):
                t0 = time.perf_counter()
                difeq.get_eq(paths[0], paths[1], "L+R", fused=fused, device=dev)
                torch.cuda.synchronize(dev)
                if i:
                    ts[fused].append((time.perf_counter() - t0) * 1e3)
        return {"samples": n, "channels": 2, "sample_rate": sr, "fused": stats(ts[True]), "composed": stats(ts[False])}
    finally:
        for p in paths:
            os.remove(p)
        os.rmdir(tmp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--skip-long", action="store_true", help="leave the 60-minute shape out (5.5 GB of samples)")
    ap.add_argument("--skip-files", action="store_true", help="leave get_eq file to file out")
    a = ap.parse_args()
    dev = 0
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(dev), "channels": 2, "reps": a.reps}
    for name, n_fft, hop, sr, seconds in SHAPES:
        if a.skip_long and seconds > 600:
            continue
        sig = noise(sr * seconds, 2, dev)
        res[name] = dict(measure(sig, n_fft, hop, a.reps, dev), sample_rate=sr, seconds=seconds)
        del sig
        torch.cuda.empty_cache()
        print(json.dumps({name: res[name]}), flush=True)
    if not a.skip_files:
        res["get_eq_files"] = measure_files(5, dev)
        print(json.dumps({"get_eq_files": res["get_eq_files"]}), flush=True)
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
