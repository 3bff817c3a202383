"""Dynamics-matcher timings (NOTES.md "Dynamics matcher"): every kernel of csrc/dynamics.hip alone, the whole
decompressor.match_dynamics_dev with the band-pass's share of it, and the composition the library allowed before these kernels
-- the same band-pass, then torch unfold / mean for the windowed RMS, torch means for the level match, a reflected conv1d for the
box filter and torch arithmetic for the overlap-add weights, the gain, the interpolation and the product.

    python tools/bench_decompressor.py [--reps 10] [--composed-reps 3] [--minutes 10] [--json profiles/decompressor_bench.json]

Signals: a 10-min 44.1 kHz stereo pair built on the device (noise whose level moves in steps; ref = src times a stepped gain),
resident in HBM.  Times are HIP-event intervals of warm calls: median, minimum and maximum of the repeats.  From the shapes:
K_wrms moves 8 rows n + 8 rows F bytes and K_dynapply 8 n ch + 8 ch F, reported as a share of the 8 TB/s HBM roofline."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyaudiorestoration_amd import _dev, _lib, decompressor as P, filters  # noqa: E402

SR, CH = 44100, 2
HOP, SZ, CORR_SZ, SMOOTHING_SEC, LOWER, UPPER = 32, 512, 4096, 0.08, 80, 9000
HBM_BYTES_PER_S = 8.0e12


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


def make_pair(n, dev):
    g = torch.Generator(device=f"cuda:{dev}").manual_seed(7)
    steps = -(-n // 50000)
    level = 10.0 ** (-torch.randint(0, 9, (steps,), generator=g, device=f"cuda:{dev}").to(torch.float32) / 4.0)
    src = (0.25 * torch.randn((n, CH), generator=g, device=f"cuda:{dev}") * level.repeat_interleave(50000)[:n, None]).contiguous()
    gain = 2.0 ** torch.randint(-3, 2, (-(-n // 70001),), generator=g, device=f"cuda:{dev}").to(torch.float32)
    ref = (src * gain.repeat_interleave(70001)[:n, None]).contiguous()
    return src, ref


def band_rows(src, ref, dev):
    n, ch = src.shape
    rows = _dev.empty((2 * ch, n), torch.float64, dev)
    rows[:ch].copy_(src.T)
    rows[ch:].copy_(ref.T)
    return rows


def composed_curves(band, ns):
    """steps 2-4 with torch: (2 ch, n) band-passed rows -> smoothed (a, b), each (ch, F)"""
    rows, n = band.shape
    F = -(-n // HOP)
    pad = (F - 1) * HOP + SZ - n
    count = torch.clamp(n - torch.arange(F, device=band.device, dtype=torch.float64) * HOP, max=SZ)
    curves = torch.empty((rows, F), dtype=torch.float64, device=band.device)
    for r in range(rows):                                                # a row at a time: the unfolded squares are 8 sz F bytes
        y = torch.nn.functional.pad(band[r], (0, pad))
        curves[r] = torch.log10(torch.clamp(torch.sqrt(y.unfold(0, SZ, HOP).square().sum(-1) / count), min=P.RMS_FLOOR))
    ch = rows // 2
    a, b = curves[:ch], curves[ch:]
    b = b - b.mean(dim=1, keepdim=True) + a.mean(dim=1, keepdim=True)
    both = torch.cat((a, b))
    lo, hi = ns // 2, ns - ns // 2 - 1
    ext = torch.cat((both[:, :lo].flip(1), both, both[:, F - hi:].flip(1)), dim=1)
    kernel = torch.full((1, 1, ns), 1.0 / ns, dtype=torch.float64, device=band.device)
    sm = torch.nn.functional.conv1d(ext[:, None, :], kernel)[:, 0, :]
    return sm[:ch], sm[ch:]


def composed_rest(src, a, b, w1, w2):
    """steps 5-8 with torch"""
    n, ch = src.shape
    F = a.shape[1]
    al = a * w1 + a * w2
    fac = torch.nan_to_num(torch.clamp(torch.pow(10.0, b) / torch.pow(10.0, al), 0.0, 2.0))
    i = torch.arange(n, device=src.device)
    j = torch.div(i, HOP, rounding_mode="floor")
    off = (i - j * HOP).to(torch.float64)
    j1 = torch.clamp(j + 1, max=F - 1)
    g = ((fac[:, j1] - fac[:, j]) / HOP * off + fac[:, j]).mean(dim=0)
    return (src.to(torch.float64) * g[:, None]).to(torch.float32)


def overlap_weights(F, dev):
    """the two Hann values each frame is multiplied by (0 where the reference has no window)"""
    ch, hann = CORR_SZ // 2, np.hanning(CORR_SZ)
    i = np.arange(F)
    K, k1, m = (F - 1) // ch, i // ch + 1, i % ch
    w1 = np.where(k1 <= K, hann[m + ch], 0.0)
    w2 = np.where(k1 + 1 <= K, hann[m], 0.0)
    return _dev.to_dev(w1, torch.float64, dev), _dev.to_dev(w2, torch.float64, dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--composed-reps", type=int, default=3)
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--json", default=None)
    ap.add_argument("--commit", default=None, help="recorded in the JSON: the commit the numbers were measured on")
    a = ap.parse_args()
    dev = 0
    torch.cuda.set_device(dev)
    n = int(a.minutes * 60 * SR)
    F, ns = P.n_frames(n, HOP), P.smoothing_size(SR, SMOOTHING_SEC, HOP)
    L, stream = _lib.lib(), _dev.stream_ptr(dev)
    src, ref = make_pair(n, dev)
    res = {"command": f"python tools/bench_decompressor.py --reps {a.reps} --composed-reps {a.composed_reps} --minutes {a.minutes:g}",
           "commit": a.commit, "samples": n, "sample_rate": SR, "channels": CH, "frames": F, "smoothing_frames": ns}

    rows = band_rows(src, ref, dev)
    res["bandpass"] = timed(lambda: filters.bandpass_batch_dev(rows, LOWER, UPPER, SR, order=P.ORDER, dev=dev), a.reps, dev)
    band = filters.bandpass_batch_dev(rows, LOWER, UPPER, SR, order=P.ORDER, dev=dev)
    del rows
    curves = _dev.empty((2 * CH, F), torch.float64, dev)
    res["k_wrms"] = timed(lambda: P.windowed_rms_dev(band, HOP, SZ, P.RMS_FLOOR, True, dev, out=curves), a.reps, dev)
    matched = curves.clone()
    res["k_level"] = timed(lambda: _lib.check(L.par_level_match_f64(dev, _dev.ptr(curves[:CH]), _dev.ptr(curves[CH:]), CH, F,
                                                                    _dev.ptr(matched[CH:]), stream)), a.reps, dev)
    smooth = torch.empty_like(matched)
    res["k_box"] = timed(lambda: _lib.check(L.par_uniform_filter_reflect_f64(dev, _dev.ptr(matched), 2 * CH, F, ns, _dev.ptr(smooth), stream)),
                         a.reps, dev)
    fac = _dev.empty((CH, F), torch.float64, dev)
    hann = P._hann_dev(CORR_SZ, dev)
    res["k_dynfac"] = timed(lambda: _lib.check(L.par_dynamics_factor_f64(dev, _dev.ptr(smooth[:CH]), _dev.ptr(smooth[CH:]), CH, F, _dev.ptr(hann),
                                                                         CORR_SZ, None, _dev.ptr(fac), stream)), a.reps, dev)
    out = _dev.empty((n, CH), torch.float32, dev)
    res["k_dynapply"] = timed(lambda: _lib.check(L.par_dynamics_apply_f32(dev, _dev.ptr(src), CH, CH, n, _dev.ptr(fac), F, HOP, _dev.ptr(out), CH,
                                                                          stream)), a.reps, dev)
    res["k_wrms_bytes"] = 8.0 * 2 * CH * n + 8.0 * 2 * CH * F
    res["k_dynapply_bytes"] = 8.0 * n * CH + 8.0 * CH * F
    res["k_wrms_share_hbm_roofline"] = res["k_wrms_bytes"] / (res["k_wrms"]["ms_min"] * 1e-3) / HBM_BYTES_PER_S
    res["k_dynapply_share_hbm_roofline"] = res["k_dynapply_bytes"] / (res["k_dynapply"]["ms_min"] * 1e-3) / HBM_BYTES_PER_S

    # the composition without the new kernels, on the same band-passed rows
    w1, w2 = overlap_weights(F, dev)
    res["composed_steps_2_to_4"] = timed(lambda: composed_curves(band, ns), a.composed_reps, dev)
    ca, cb = composed_curves(band, ns)
    res["composed_steps_5_to_8"] = timed(lambda: composed_rest(src, ca, cb, w1, w2), a.composed_reps, dev)
    cout = composed_rest(src, ca, cb, w1, w2)
    res["composed_max_abs_diff_vs_kernels"] = float((cout.to(torch.float64) - out.to(torch.float64)).abs().max())
    res["output_peak"] = float(out.abs().max())
    del band, ca, cb, cout, curves, matched, smooth
    kernels_ms = sum(res[k]["ms_median"] for k in ("k_wrms", "k_level", "k_box", "k_dynfac", "k_dynapply"))
    composed_ms = res["composed_steps_2_to_4"]["ms_median"] + res["composed_steps_5_to_8"]["ms_median"]
    res["kernels_ms_median_sum"] = kernels_ms
    res["composed_ms_median_sum"] = composed_ms
    res["ratio_composed_over_kernels"] = composed_ms / kernels_ms

    res["match_dynamics_dev"] = timed(lambda: P.match_dynamics_dev(src, ref, SR, dev=dev), a.reps, dev)
    res["bandpass_share_of_match_dynamics"] = res["bandpass"]["ms_median"] / res["match_dynamics_dev"]["ms_median"]
    print(json.dumps(res), flush=True)
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
