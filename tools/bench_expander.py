"""Spectral Expander timings (NOTES.md "Spectral Expander"): the band curve fused (par_stft_band_db_f32) against composed (magnitude
rows of frame chunks + par_band_mean_db_f32), volume_curves, expand on the device, and expand_file-shaped numpy -> numpy.

    python tools/bench_expander.py [--reps 10] [--json out.json]

Files: 10 min at 44.1 kHz stereo and 60 min at 192 kHz mono (691.2 M samples), synthetic, built on the device.  Device times are
HIP-event intervals of warm calls (median of --reps); kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of
this script.  Algorithmic bytes from the shapes: fused = 4 B per sample read + 8 B per frame written; composed additionally writes
the magnitude rows (4 B x bins per frame, 16 B per input sample at hop 64) and reads the band rows back."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyaudiorestoration_amd import _dev, expander, spectrum_flat  # noqa: E402

FILES = {"10min_44k1_stereo": (26_460_000, 44100, 2), "60min_192k_mono": (691_200_000, 192000, 1)}


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
    ap.add_argument("--json", default=None)
    ap.add_argument("--files", default=",".join(FILES))
    a = ap.parse_args()
    dev = 0
    torch.cuda.set_device(dev)
    res = {}
    for name in a.files.split(","):
        n, sr, ch = FILES[name]
        g = torch.Generator(device=f"cuda:{dev}").manual_seed(1)
        x_t = torch.randn((n, ch), generator=g, device=f"cuda:{dev}", dtype=torch.float32).mul_(1e-3)
        flat = x_t.reshape(-1)
        frames = n // 64 + 1
        bl, bu = expander.freq2bin(13000, 257, 512, sr), expander.freq2bin(17000, 257, 512, sr)
        out = _dev.empty(frames, torch.float64, dev)
        r = {"samples": n, "channels": ch, "frames": frames, "band_bins": bu - bl}
        for fused in (True, False):
            def curve():
                for c in range(ch):
                    spectrum_flat.band_db_curve_dev(flat[c:], 512, 64, bl, bu, x_stride=ch, n=n, fused=fused, dev=dev, out=out)
            med, best = timed(curve, a.reps, dev)
            key = "fused" if fused else "composed"
            nbytes = ch * (4 * n + 8 * frames) + (0 if fused else ch * frames * (4 * 257 + 4 * (bu - bl)))
            r[f"curve_{key}_ms"], r[f"curve_{key}_best_ms"] = med, best
            r[f"curve_{key}_alg_GBps"] = nbytes / (best * 1e-3) / 1e9
            r[f"curve_{key}_alg_bytes"] = nbytes
        r["volume_curves_ms"] = timed(lambda: expander.volume_curves(x_t, sr, device=dev), a.reps, dev)[0]
        curves, _ = expander.volume_curves(x_t, sr, device=dev)
        r["expand_dev_ms"] = timed(lambda: expander.expand(x_t, sr, curves, device=dev), a.reps, dev)[0]
        r["expand_dev_transition_ms"] = timed(lambda: expander.expand(x_t, sr, curves, transition=4000, order=2, device=dev),
                                              max(2, a.reps // 3), dev)[0]
        host = x_t.cpu().numpy()
        del x_t, flat
        torch.cuda.empty_cache()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            s_t = _dev.to_dev(host, torch.float32, dev)
            cv, _ = expander.volume_curves(s_t, sr, device=dev)
            y = _dev.to_host(expander.expand(s_t, sr, cv, device=dev))
            ts.append(time.perf_counter() - t0)
            del s_t, y
        r["expand_file_np_to_np_s"] = float(np.median(ts))
        r["expand_file_np_to_np_Msps"] = n / r["expand_file_np_to_np_s"] / 1e6
        res[name] = r
        print(name, json.dumps(r), flush=True)
        del host
        torch.cuda.empty_cache()
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
