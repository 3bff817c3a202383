"""Cyclic wow timings (NOTES.md "Cyclic wow"): the pilot track of one channel by

  fused      par_stft_track_peak_f64 (cyclic_wow.pilot_track, fused=True): band argmax and parabola inside the transform kernel,
             one float64 per frame leaves it; no spectrogram stored
  composed   fourier.stft_dev mode 1 over frame chunks of 512 MB, float32 dB on the device, par_track_peak_f64 per chunk
             (fused=False): the parent's kernels

at 16384 / 128 (the tool's setting) on 1 min and on 20 min at 44.1 kHz, and at 4096 / 32 on 10 min; cycle_search
(par_cycle_fold_f64, all candidates in one launch) for the 20-minute track against the numpy loop of the reference; and
cyclic_wow.analyse file to file on the 20-minute file with either path.

    python tools/bench_cyclic.py [--reps 20] [--json profiles/cyclic_bench.json] [--skip-long] [--skip-files]

Protocol (that of tools/bench_difeq.py): the signal is a synthetic pilot with a cyclic speed error, resident in HBM.  After two warm
calls of each path, fused and composed alternate for `reps` rounds in one process, every whole Python call timed by HIP events
around it; the medians are reported.  Then the composed path is repeated alone in three more series of `reps` calls: `spread_ms`
is the distance between the largest and the smallest of its four medians.  `fused_ahead` is fused median + spread < composed
median.  A shape whose composed call takes more than 1.5 s is measured with 5 rounds instead (said in `reps`).  analyse is
wall-clock time (file reading, upload, track, download, search), median of 3 alternating calls."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyaudiorestoration_amd import _lib, cyclic_wow, io_ops  # noqa: E402

SR, RPM, PILOT = 44100, 33.333, 3150.0
SHAPES = (("tool_1min", 16384, 128, 60), ("tool_20min", 16384, 128, 1200), ("small_10min", 4096, 32, 600))


def pilot(seconds, dev):
    """float32 (n,) on the device: the pilot with +-0.3 % of cyclic speed error at RPM, and a little noise"""
    n = SR * seconds
    t = torch.arange(n, dtype=torch.float64, device=f"cuda:{dev}") / SR
    speed = 1.0 + 0.003 * torch.sin(2 * np.pi * t * (RPM / 60.0))
    phase = 2 * np.pi * PILOT * torch.cumsum(speed, 0) / SR
    g = torch.Generator(device=f"cuda:{dev}").manual_seed(11)
    return (0.5 * torch.sin(phase) + 1e-3 * torch.randn(n, generator=g, device=f"cuda:{dev}", dtype=torch.float64)).to(torch.float32)


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
    n = sig.shape[0]
    trail = [(0.0, PILOT), (n / SR, PILOT)]
    fused = lambda: cyclic_wow.pilot_track(sig, SR, list(trail), n_fft, hop, fused=True, device=dev)
    composed = lambda: cyclic_wow.pilot_track(sig, SR, list(trail), n_fft, hop, fused=False, device=dev)
    a, b = fused()[1], composed()[1]
    fused(), composed()
    torch.cuda.synchronize(dev)
    if once(composed, dev) > 1500.0:
        reps = min(reps, 5)
    tf, tc = [], []
    for _ in range(reps):
        tf.append(once(fused, dev))
        tc.append(once(composed, dev))
    alone = [[once(composed, dev) for _ in range(reps)] for _ in range(3)]
    medians = [float(np.median(tc))] + [float(np.median(s)) for s in alone]
    spread = max(medians) - min(medians)
    frames, bins = int(_lib.lib().par_stft_frames(n, n_fft, hop)), n_fft // 2 + 1
    return {"samples": n, "fft_size": n_fft, "hop": hop, "frames": frames, "fused": stats(tf), "composed": stats(tc),
            "composed_alone_medians_ms": medians[1:], "spread_ms": spread, "ratio_composed_over_fused": float(np.median(tc) / np.median(tf)),
            "fused_ahead": bool(np.median(tf) + spread < np.median(tc)),
            "fused_minus_composed_max_abs_hz": float(np.max(np.abs(a - b))),
            "fused_algorithmic_bytes": int(n * 4 + frames * 16),
            "composed_algorithmic_bytes": int(n * 4 + frames * bins * 4 * 4 + frames * 16)}, a


def measure_search(freqs, hop, reps, dev):
    logf = np.log2(freqs)
    frames_init = int(60.0 / RPM * SR / hop)
    logf_t = torch.from_numpy(logf).to(f"cuda:{dev}")
    gpu = lambda: cyclic_wow.cycle_search(logf_t, frames_init, 0.1, dev)
    res = gpu()
    gpu()
    tg = [once(gpu, dev) for _ in range(reps)]

    def loop():
        d = int(frames_init * 0.1)
        out = np.empty((2 * d, 2))
        for i in range(-d, d):
            P = frames_init + i
            V = len(logf) // P
            avg = np.mean(np.split(logf[:V * P], V), axis=0)
            out[d + i] = (P, np.max(avg) - np.min(avg))
        return out
    tn = []
    for _ in range(5):
        t0 = time.perf_counter()
        ref = loop()
        tn.append((time.perf_counter() - t0) * 1e3)
    return {"frames": len(logf), "frames_init": frames_init, "candidates": len(res), "gpu": stats(tg), "numpy_loop": stats(tn),
            "equal_bit_for_bit": bool(np.array_equal(res, ref)), "best": [float(v) for v in res[np.argmax(res[:, 1])]]}


def measure_files(sig, reps, dev):
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "side.wav")
    try:
        io_ops.write_wav_float(path, sig.cpu().numpy(), SR)
        ts = {True: [], False: []}
        for i in range(reps + 1):
            for fused in (True, False):
                t0 = time.perf_counter()
                res = cyclic_wow.analyse(path, rpm=RPM, pilot_hz=PILOT, fused=fused, device=dev)
                torch.cuda.synchronize(dev)
                if i:
                    ts[fused].append((time.perf_counter() - t0) * 1e3)
        return {"samples": int(sig.shape[0]), "sample_rate": SR, "fused": stats(ts[True]), "composed": stats(ts[False]),
                "report": cyclic_wow.report(res)}
    finally:
        os.remove(path)
        os.rmdir(tmp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--skip-long", action="store_true", help="leave the 20-minute shape (and what hangs on it) out")
    ap.add_argument("--skip-files", action="store_true", help="leave analyse file to file out")
    a = ap.parse_args()
    dev = 0
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(dev), "sample_rate": SR, "reps": a.reps}
    for name, n_fft, hop, seconds in SHAPES:
        if a.skip_long and seconds > 600:
            continue
        sig = pilot(seconds, dev)
        res[name], freqs = measure(sig, n_fft, hop, a.reps, dev)
        res[name]["seconds"] = seconds
        print(json.dumps({name: res[name]}), flush=True)
        if name == "tool_20min":
            res["cycle_search_20min"] = measure_search(freqs, hop, a.reps, dev)
            print(json.dumps({"cycle_search_20min": res["cycle_search_20min"]}), flush=True)
            if not a.skip_files:
                res["analyse_files_20min"] = measure_files(sig, 3, dev)
                print(json.dumps({"analyse_files_20min": res["analyse_files_20min"]}), flush=True)
        del sig
        torch.cuda.empty_cache()
        if a.json:
            json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
