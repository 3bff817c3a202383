"""Zero-crossing flutter timings (NOTES.md "Zero-crossing flutter"): from the compacted sign changes of a pilot tone to the pitch
curve on a regular grid, by

  device   zerocrossing_wow.smooth_crossings_dev (two crossing indices read back for the span, the Hann weights uploaded,
           par_crossing_smooth_f64) and interp_dev (par_interp_f64) onto the grid, the grid downloaded
  host     today's tail of ZeroCrossingTracker.trace: all crossings downloaded (.cpu().numpy()), then
           wow_detection.crossing_periods_to_freqs (np.diff, reflect pad, np.convolve, division, np.interp) on one core

on synthetic pilots of 1, 10 and 60 minutes at 192 kHz with a 4 kHz pilot, the grid every 256 samples.

    python tools/bench_zerocrossing.py [--minutes 1,10,60] [--reps 10] [--host-reps 3] [--json profiles/zerocrossing_bench.json]

Protocol: the signal is synthesised in HBM and its sign changes are compacted once (par_zero_crossings_f64; common to both paths,
not timed).  After two warm calls the device chain and the host tail alternate; a whole call is wall-clock time around work that
ends in a device synchronise (device) or on the host (host), the median is reported.  The two kernels are then timed alone with
HIP events around the C entry points, `reps` launches each.  `algorithmic_bytes` is what the kernels must move, computed from the
shapes: K_zcsmooth reads 8 bytes per crossing and writes 8 + 8 + 4 per period; K_interp reads and writes 8 bytes per grid point
(its table look-ups hit the cache).  The device and the host curves are compared on the grid."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyaudiorestoration_amd import _dev, _lib, wow_detection, zerocrossing_wow as zc  # noqa: E402

SR, PILOT, HOP = 192000, 4000.0, 256


def crossings_of_pilot(seconds, dev):
    """device int64 crossings of a 4 kHz pilot with +-1 % flutter at 9 Hz and a little noise, and the number of samples"""
    n = SR * seconds
    t = torch.arange(n, dtype=torch.float64, device=f"cuda:{dev}") / SR
    phase = 2 * np.pi * PILOT * (t - 0.01 / (2 * np.pi * 9.0) * torch.cos(2 * np.pi * 9.0 * t))       # the integral of the speed
    del t
    g = torch.Generator(device=f"cuda:{dev}").manual_seed(17)
    x = torch.sin(phase)
    del phase
    x.mul_(0.5).add_(torch.randn(n, generator=g, device=f"cuda:{dev}", dtype=torch.float32), alpha=1e-3)
    c = wow_detection.zero_crossings_dev(x, dev)
    del x
    torch.cuda.empty_cache()
    return c, n


def stats(ts):
    return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "reps": len(ts)}


def events(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def measure(seconds, reps, host_reps, dev):
    c_t, n_samples = crossings_of_pilot(seconds, dev)
    grid = zc.grid(n_samples, SR, HOP)
    grid_t = _dev.to_dev(grid, torch.float64, dev)

    def device_chain():
        sm = zc.smooth_crossings_dev(c_t, SR)
        return sm, zc.interp_dev(grid_t, sm.xp, sm.freq).cpu().numpy()

    def host_tail():
        t0 = time.perf_counter()
        crossings = c_t.cpu().numpy()
        t1 = time.perf_counter()
        return wow_detection.crossing_periods_to_freqs(crossings, SR, 0.0, grid), (t1 - t0) * 1e3

    sm, got = device_chain()
    device_chain()
    want, _ = host_tail()
    td, th, tdl = [], [], []
    for i in range(max(reps, host_reps)):
        if i < reps:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            device_chain()
            torch.cuda.synchronize(dev)
            td.append((time.perf_counter() - t0) * 1e3)
        if i < host_reps:
            t0 = time.perf_counter()
            _, dl = host_tail()
            th.append((time.perf_counter() - t0) * 1e3)
            tdl.append(dl)
    # the kernels alone
    L = _lib.lib()
    c, n, span = c_t.numel(), c_t.numel() - 1, sm.span
    kernel_t = _dev.to_dev(zc.hann_kernel(span), torch.float64, dev)
    xp, freq, raw = _dev.empty(n, torch.float64, dev), _dev.empty(n, torch.float64, dev), _dev.empty(n, torch.float32, dev)
    out = _dev.empty(len(grid), torch.float64, dev)
    smooth = lambda: _lib.check(L.par_crossing_smooth_f64(dev, _dev.ptr(c_t), c, _dev.ptr(kernel_t), span, float(SR), 0.0, None, _dev.ptr(freq),
                                                          _dev.ptr(xp), _dev.ptr(raw), _dev.stream_ptr(dev)))
    interp = lambda: _lib.check(L.par_interp_f64(dev, _dev.ptr(grid_t), len(grid), _dev.ptr(xp), _dev.ptr(freq), n, _dev.ptr(out),
                                                 _dev.stream_ptr(dev)))
    for fn in (smooth, interp, smooth, interp):
        fn()
    ts, ti = [events(smooth, dev) for _ in range(reps)], [events(interp, dev) for _ in range(reps)]
    smooth_bytes, interp_bytes = c * 8 + n * 20, len(grid) * 16
    return {"seconds": seconds, "samples": n_samples, "crossings": c, "span": span, "grid_points": len(grid),
            "device_whole_call": stats(td), "host_tail": stats(th), "host_tail_download_ms_median": float(np.median(tdl)),
            "ratio_host_over_device": float(np.median(th) / np.median(td)),
            "k_zcsmooth": dict(stats(ts), algorithmic_bytes=smooth_bytes, gb_per_s=smooth_bytes / np.median(ts) / 1e6,
                               taps_per_s=n * span / np.median(ts) * 1e3),
            "k_interp": dict(stats(ti), algorithmic_bytes=interp_bytes),
            "crossings_download_bytes": c * 8, "device_download_bytes": len(grid) * 8 + 16,
            "device_minus_host_max_rel": float(np.max(np.abs(got - want) / want)),
            "bound_2_span_plus_4_plus_4_u": (2 * (span + 4) + 4) * 2.0 ** -53}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=lambda s: [int(v) for v in s.split(",")], default=[1, 10, 60])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = 0
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(dev), "sample_rate": SR, "pilot_hz": PILOT, "hop": HOP}
    for minutes in a.minutes:
        name = f"pilot_{minutes}min"
        res[name] = measure(60 * minutes, a.reps, a.host_reps, dev)
        print(json.dumps({name: res[name]}), flush=True)
        torch.cuda.empty_cache()
        if a.json:
            json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
