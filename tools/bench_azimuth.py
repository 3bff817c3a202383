"""Tape-sync azimuth mode timings (NOTES.md "Tape-sync azimuth lines"): pipeline.azimuth_line against the loop over
pipeline.correlate_sources(..., window_name="hann") it replaces -- the only way the library offered before -- and every stage of the
batch alone.

    python tools/bench_azimuth.py [--reps 5] [--loop-reps 2] [--seconds 10] [--json profiles/azimuth_bench.json]

Per sample rate (44.1 kHz and 192 kHz): a synthetic file from tests/inputs.bench_signal and the same take 3.3 ms later with 1 % of
noise, a selection of --seconds at the GUI's defaults (win 0.2 s, overlap 32: 160 windows per second of 2 x 0.2 s each), band
300 .. 5000 Hz.  azimuth_line and the loop are host wall-clock times around calls that end in a device-to-host copy (they include
the host's share: geometry, filter design, launches); the loop gets the windows already cut.  The stages are HIP-event intervals of
warm calls on the largest group of windows.  Median, minimum and maximum of the repeats; the device's clocks as rocm-smi reports them
before and after.  The two paths' results are compared bit for bit on the windows timed."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import inputs  # noqa: E402
from pyaudiorestoration_amd import _dev, correlation, filters, pipeline  # noqa: E402

DUR, OVERLAP, REJECT, LOWER, UPPER, T0 = 0.2, 32, 0.1, 300.0, 5000.0, 2.0


def stats(ts):
    return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "reps": len(ts)}


def wall(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return stats(ts)


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return stats(ts)


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0", "--json"], capture_output=True, text=True, timeout=30).stdout
        return json.loads(out)
    except Exception as e:                       # the figures stand without it; say so in the record
        return {"unavailable": repr(e)}


def make_files(sr, seconds):
    n = int((seconds + 2 * T0) * sr)
    ref = inputs.bench_signal(0, n + 64, sr).astype(np.float64)
    lag = 0.0033 * sr
    src = np.interp(np.arange(n) + lag, np.arange(len(ref)), ref) + 0.01 * np.random.default_rng(5).standard_normal(n)
    return ref[:n].astype(np.float32), src.astype(np.float32)


def bench_rate(sr, a):
    dev = 0
    ref, src = make_files(sr, a.seconds)
    t0, t1 = T0, T0 + a.seconds
    curve = np.array([[0.0, 0.003], [1000.0, 0.003]])
    times, lags, ref_geom, src_geom = pipeline.azimuth_windows(len(ref), len(src), sr, t0, t1, curve, DUR, OVERLAP)
    W = len(times)
    cut = lambda sig, g: np.concatenate((np.zeros(g[2], sig.dtype), sig[g[0]:g[0] + g[1]], np.zeros(g[3], sig.dtype)))
    wins = [(cut(ref, ref_geom[i]), cut(src, src_geom[i])) for i in range(W)]
    shapes = {}
    for i, (x, y) in enumerate(wins):
        shapes.setdefault((len(x), len(y)), []).append(i)
    res = {"sample_rate": sr, "windows": W, "shapes": {f"{k[0]}x{k[1]}": len(v) for k, v in shapes.items()}}

    line = {}

    def batch():
        line["v"] = pipeline.azimuth_line(ref, src, sr, t0, t1, LOWER, UPPER, curve, DUR, OVERLAP, REJECT)
    res["azimuth_line"] = wall(batch, a.reps)
    ref_t, src_t = _dev.to_dev(ref, torch.float32, dev), _dev.to_dev(src, torch.float32, dev)

    def batch_resident():
        pipeline.azimuth_line(ref_t, src_t, sr, t0, t1, LOWER, UPPER, curve, DUR, OVERLAP, REJECT)
    res["azimuth_line_files_resident"] = wall(batch_resident, a.reps)

    loop = {"raw": np.empty(W), "corr": np.empty(W)}

    def looped():
        for i, (x, y) in enumerate(wins):
            d, loop["corr"][i] = pipeline.correlate_sources(x, y, sr, LOWER, UPPER, False, "hann")
            loop["raw"][i] = lags[i] + d
    res["loop_correlate_sources"] = wall(looped, a.loop_reps)
    res["loop_ms_per_window"] = res["loop_correlate_sources"]["ms_median"] / W
    res["batch_ms_per_window"] = res["azimuth_line"]["ms_median"] / W
    res["loop_over_batch"] = res["loop_correlate_sources"]["ms_median"] / res["azimuth_line"]["ms_median"]
    same = lambda p, q: bool(np.array_equal(np.asarray(p).view(np.uint64), np.asarray(q).view(np.uint64)))
    res["bit_equal_to_loop"] = same(line["v"].lags_raw, loop["raw"]) and same(line["v"].corrs, loop["corr"])

    # the stages on the largest group, as azimuth_line issues them
    (na, nb), idx = max(shapes.items(), key=lambda kv: len(kv[1]))
    idx = np.asarray(idx)
    per_window = correlation.batch_scratch_bytes(na, nb, 1) + 5 * 8 * (na + nb)
    idx = idx[:int(max(1, min(len(idx), (1 << 30) // per_window)))]
    res["stage_windows"], res["stage_shape"] = len(idx), [na, nb]
    g = lambda: (pipeline.gather_windows_dev(ref_t, 1, len(ref), 0, ref_geom[idx], na, dev),
                 pipeline.gather_windows_dev(src_t, 1, len(src), 0, src_geom[idx], nb, dev))
    res["stage_gather_both"] = events(g, a.reps)
    a_t, b_t = g()
    res["stage_filter_ref"] = events(lambda: filters.bandpass_batch_dev(a_t, LOWER, UPPER, sr, order=3, dev=dev), a.reps)
    res["stage_filter_src"] = events(lambda: filters.bandpass_batch_dev(b_t, LOWER, UPPER, sr, order=3, dev=dev), a.reps)
    a_f = filters.bandpass_batch_dev(a_t, LOWER, UPPER, sr, order=3, dev=dev)
    b_f = filters.bandpass_batch_dev(b_t, LOWER, UPPER, sr, order=3, dev=dev)
    keep_a, keep_b = a_f.clone(), b_f.clone()

    def search():                                # the window is applied in place: every repeat starts from the filtered rows
        a_f.copy_(keep_a)
        b_f.copy_(keep_b)
        correlation.find_delay_batch_dev(a_f, b_f, False, "hann", dev)
    res["stage_delay_search_with_row_restore"] = events(search, a.reps)
    res["stage_row_restore"] = events(lambda: (a_f.copy_(keep_a), b_f.copy_(keep_b)), a.reps)
    N = 8192
    while N < na + nb - 1:
        N <<= 1
    # bytes the search moves per window, from the shapes: the in-place window (read + write), the norms and the packing read the rows
    # (32 (na + nb)); the packed array is written once, goes through two transforms of two passes (read + write each) and the cross
    # spectrum (88 N); the 'same' span is read twice as float2 (16 na); seven exact sums read nb samples of both rows (112 nb)
    res["delay_search_bytes_per_window"] = 32 * (na + nb) + 88 * N + 16 * na + 112 * nb
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-reps", type=int, default=2)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rates", type=lambda s: [int(v) for v in s.split(",")], default=[44100, 192000])
    ap.add_argument("--json", default=None)
    ap.add_argument("--commit", default=None, help="recorded in the JSON: the commit the numbers were measured on")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm GPU visible; nothing is measured without one")
    torch.cuda.set_device(0)
    res = {"command": f"python tools/bench_azimuth.py --reps {a.reps} --loop-reps {a.loop_reps} --seconds {a.seconds:g}", "commit": a.commit,
           "device": torch.cuda.get_device_name(0), "win_s": DUR, "overlap": OVERLAP, "band_hz": [LOWER, UPPER],
           "clocks_before": clocks(), "rates": []}
    for sr in a.rates:
        res["rates"].append(bench_rate(sr, a))
        print(json.dumps(res["rates"][-1]), flush=True)
    res["clocks_after"] = clocks()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
