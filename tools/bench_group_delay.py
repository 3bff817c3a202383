"""Group-delay timings (NOTES.md "Group delay"): group_delay.measure on stereo noise pairs of 10 s, 60 s and 180 s at 44.1 kHz, 43 bands,
and its two stages on the same filtered rows:

  whole     group_delay.measure(ref, src, sr), upload and read-back included
  filter    filters.bandpass_batch_dev on the replicated rows of one chunk of bands
  sect      correlation.find_delay_rows_dev (par_find_delay_sect_f64) on that chunk's filtered rows, one call
  loop      correlation.find_delay (par_find_delay_f64) band by band over the SAME rows: one pair per call, a host wait each

    python tools/bench_group_delay.py [--seconds 10,60,180] [--reps 5] [--json profiles/group_delay_bench.json] [--check]

Protocol: the pair is synthesised once (seeded), every stage runs twice before it is timed, `sect` and `loop` alternate in one process,
a time is wall clock around work that ends in a device synchronise; median, minimum and maximum of `reps` runs are reported.  The chunk is
the number of bands group_delay.measure itself sends through at its default max_bytes.  `transforms` are counted from the shapes
(2^20-point transforms per band: 2 P Q pair by pair, max(P, Q) + P + Q - 1 by diagonals), not measured.
--check measures the worst lag error of same_out at S = 2^19, P = Q = 16 against scipy's float64 FFT correlation and prints twice that
error beside kXcRivalTol."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.signal
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyaudiorestoration_amd import correlation, filters, group_delay  # noqa: E402

SR = 44100
RIVAL_TOL = 4.0e-6              # kXcRivalTol


def pair(n, seed=3):
    rng = np.random.default_rng([93, n, seed])
    ref = rng.standard_normal(n).astype(np.float32)
    sos = scipy.signal.bessel(1, 300, "low", analog=False, output="sos", fs=SR)
    src = np.roll(scipy.signal.sosfilt(sos, ref.astype(np.float64)), 7) + 0.02 * rng.standard_normal(n)
    return ref, src.astype(np.float32)


def stats(ts):
    return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "reps": len(ts)}


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def transforms(n):
    S = 1 << 19
    if 2 * n - 1 <= (1 << 20):
        return {"P": 1, "Q": 1, "pair_by_pair": 2, "diagonals": 2}
    P = -(-n // S)
    return {"P": P, "Q": P, "pair_by_pair": 2 * P * P, "diagonals": P + 2 * P - 1}


def measure(seconds, reps, dev):
    n = SR * seconds
    ref, src = pair(n)
    edges = group_delay.band_limits()
    lo, hi = edges[:-1].astype(np.float64), edges[1:].astype(np.float64)
    n_bands = len(lo)
    chunk = min(n_bands, max(1, int(((4 << 30) // 2) // (8 * 2 * n * 4))))     # group_delay.measure's own chunk at its default max_bytes
    ref_t, src_t = (torch.from_numpy(v).to(f"cuda:{dev}").double() for v in (ref, src))
    x = torch.empty((2 * chunk, n), dtype=torch.float64, device=f"cuda:{dev}")
    x[:chunk], x[chunk:] = ref_t, src_t
    bands = (np.tile(lo[-chunk:], 2), np.tile(hi[-chunk:], 2))
    filt = lambda: filters.bandpass_batch_dev(x, bands[0], bands[1], SR, 1, dev)
    y = filt()
    ya, yb = y[:chunk], y[chunk:]
    sect = lambda: correlation.find_delay_rows_dev(ya, yb, want_norms=True)
    loop = lambda: [correlation.find_delay(ya[k], yb[k]) for k in range(chunk)]
    whole = lambda: group_delay.measure(ref, src, SR)
    for fn in (filt, sect, loop, sect, loop, whole):
        fn()
    d, c, _, _ = sect()
    same = bool(np.array_equal(d.cpu().numpy(), np.array([r[0] for r in loop()])))
    tf, ts, tl, tw = [], [], [], []
    for _ in range(reps):
        ts.append(timed(sect, dev))
        tl.append(timed(loop, dev))
        tf.append(timed(filt, dev))
    for _ in range(max(2, reps // 2)):
        tw.append(timed(whole, dev))
    scale = n_bands / chunk
    return {"seconds": seconds, "samples": n, "bands": n_bands, "bands_per_chunk": chunk, "transforms_per_band": transforms(n),
            "whole_measure": stats(tw), "filter_chunk": stats(tf), "sect_chunk": stats(ts), "loop_chunk": stats(tl),
            "sect_ms_per_band": float(np.median(ts)) / chunk, "loop_ms_per_band": float(np.median(tl)) / chunk,
            "ratio_loop_over_sect": float(np.median(tl) / np.median(ts)), "all_bands_scale": scale, "delays_bit_equal": same}


def check(dev):
    n = 16 << 19
    ref, src = pair(n, seed=4)
    a = torch.from_numpy(ref).to(f"cuda:{dev}").double()[None]
    b = torch.from_numpy(src).to(f"cuda:{dev}").double()[None]
    d, c, s, same = correlation.find_delay_rows_dev(a, b, section=19, want_same=True)
    want = scipy.signal.correlate(ref.astype(np.float64) / np.linalg.norm(ref.astype(np.float64)),
                                  src.astype(np.float64) / np.linalg.norm(src.astype(np.float64)), mode="same", method="fft")
    e = float(np.max(np.abs(same[0].cpu().numpy() - want)))
    return {"samples": n, "section_log2": 19, "P": 16, "Q": 16, "worst_lag_error": e, "twice": 2 * e, "kXcRivalTol": RIVAL_TOL,
            "precondition_holds": bool(2 * e <= RIVAL_TOL), "delay": float(d[0]), "corr": float(c[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=lambda s: [int(v) for v in s.split(",")], default=[10, 60, 180])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    dev = 0
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(dev), "sample_rate": SR}
    if a.check:
        res["check_same_out"] = check(dev)
        print(json.dumps({"check_same_out": res["check_same_out"]}), flush=True)
        torch.cuda.empty_cache()
    for seconds in a.seconds:
        name = f"pair_{seconds}s"
        res[name] = measure(seconds, a.reps, dev)
        print(json.dumps({name: res[name]}), flush=True)
        torch.cuda.empty_cache()
        if a.json:
            json.dump(res, open(a.json, "w"), indent=1)
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
