"""Fixed-ratio resampler timings (NOTES.md "Fixed-ratio resampler").

    python tools/bench_resample_fixed.py [--cases a_up,a_down,b_up,b_down] [--reps 9] [--json out.json]

K_rsfix alone (par_resample_fixed_f32, one launch per channel), timed with par_event_* on the stream the kernels run on: two
warm calls, then the median (and minimum) of --reps.  Signals are seeded noise built on the device.

  a_up    10 min stereo at 44.1 kHz -> 48 kHz            a_down  10 min stereo at 48 kHz -> 44.1 kHz
  b_up    60 min mono at 192 kHz, ratio 1.0417           b_down  60 min mono at 192 kHz, ratio 0.96

From the shapes: 4 B read + 4 B written per output, so the share of the HBM peak (8 TB/s) is 8 * outputs / time / 8e12.
As a landmark only, K_sinc (par_varispeed_fused_f32, NT = 32) on the same input with a constant speed curve (the ratio at a
point every 4096 samples, about as many outputs): another filter (the reference's own time-varying sinc), a different amount
of work per output; not a baseline to beat."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyaudiorestoration_amd import _dev, _lib, fixed_rate, resampling  # noqa: E402

CASES = {"a_up": (26_460_000, 2, 44100.0, 48000.0), "a_down": (28_800_000, 2, 48000.0, 44100.0),
         "b_up": (691_200_000, 1, 192000.0, 192000.0 * 1.0417), "b_down": (691_200_000, 1, 192000.0, 192000.0 * 0.96)}
HBM_BPS = 8.0e12           # MI355X HBM3E peak
CURVE_STEP = 4096          # samples between the points of the landmark's constant speed curve


def timed(fn, reps, dev):
    L = _lib.lib()
    ev = [ctypes.c_void_p() for _ in range(2)]
    for e in ev:
        _lib.check(L.par_event_create(ctypes.byref(e)))
    for _ in range(2):
        fn()
    torch.cuda.synchronize(dev)
    ts = []
    for _ in range(reps):
        ms = ctypes.c_float(0.0)
        _lib.check(L.par_event_record(ev[0], _dev.stream_ptr(dev)))
        fn()
        _lib.check(L.par_event_record(ev[1], _dev.stream_ptr(dev)))
        _lib.check(L.par_event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms)))
        ts.append(ms.value)
    for e in ev:
        L.par_event_destroy(e)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="a_up,a_down,b_up,b_down")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = 0
    torch.cuda.set_device(dev)
    res = {"reps": a.reps, "device": torch.cuda.get_device_name(dev)}
    for name in a.cases.split(","):
        n, ch, sr_a, sr_b = CASES[name]
        g = torch.Generator(device=f"cuda:{dev}").manual_seed(5)
        x = torch.empty((n, ch), dtype=torch.float32, device=f"cuda:{dev}")
        for s in range(0, n, 1 << 24):
            x[s:s + (1 << 24)] = torch.rand((min(1 << 24, n - s), ch), generator=g, device=f"cuda:{dev}") * 2 - 1
        n_out = fixed_rate.out_len(n, sr_a, sr_b)
        out = _dev.empty((n_out, ch), torch.float32, dev)
        med, best = timed(lambda: fixed_rate.resample_dev(x, n, ch, sr_a, sr_b, out=out, dev=dev), a.reps, dev)
        outputs = n_out * ch
        r = {"samples": n, "channels": ch, "sr_orig": sr_a, "sr_new": sr_b, "outputs": outputs, "k_rsfix_ms": med, "k_rsfix_ms_min": best,
             "gsamples_per_s": outputs / (med * 1e-3) / 1e9, "algorithmic_bytes_per_output": 8,
             "share_hbm_peak": 8.0 * outputs / (med * 1e-3) / HBM_BPS}
        del out
        try:                                       # landmark: K_sinc, constant speed curve, the existing fused path
            times_t = torch.arange(0, n + CURVE_STEP, CURVE_STEP, dtype=torch.float64, device=f"cuda:{dev}")
            speeds_t = torch.full_like(times_t, sr_b / sr_a)
            plan = resampling.speed_plan_dev(times_t, speeds_t, n, dev, fused=True)
            if not plan.fused_ok:
                raise RuntimeError("the plan refused the fused form")
            flat = x.reshape(-1)
            outs = [_dev.empty(plan.len_out, torch.float32, dev) for _ in range(ch)]
            med_s, best_s = timed(lambda: [resampling.varispeed_fused_dev(plan, flat[c:], 32, outs[c], sig_stride=ch, len_in=n) for c in range(ch)],
                                  max(a.reps // 2, 3), dev)
            r["landmark_k_sinc_nt32_ms"] = med_s
            r["landmark_k_sinc_outputs"] = plan.len_out * ch
            r["landmark_k_sinc_gsamples_per_s"] = plan.len_out * ch / (med_s * 1e-3) / 1e9
            del outs
        except Exception as e:                     # the landmark is not what this tool measures
            r["landmark_error"] = f"{type(e).__name__}: {e}"
        res[name] = r
        print(json.dumps({name: r}), flush=True)
        del x
        torch.cuda.empty_cache()
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
