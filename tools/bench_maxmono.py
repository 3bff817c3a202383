"""MaxMono timings (NOTES.md "MaxMono"): the fused kernel (par_maxmono_stft_f32, one launch) against the composed device route
stage by stage (K_stft twice -> par_select_spectrum_f32 -> K_istft twice) and against a torch.stft / torch.where / torch.istft
composition on the same GPU.

    python tools/bench_maxmono.py [--reps 10] [--json profiles/maxmono_bench.json]

File: 10 min at 44.1 kHz stereo, synthetic (two takes of a tone over independent noise), resident in HBM.  Geometries 512/64
(the GUI's default), 2048/512, 2048/128 and 8192/1024.  Times are HIP-event intervals of warm calls (median and minimum of
--reps, after one warm-up call per shape), every interval closed by a device synchronise.  From the shapes: 16 algorithmic bytes
per stereo sample (two channels read, two outputs written) against the 8 TB/s roofline, and the redundant-frame share of the
streaming kernel (par_maxmono_stft_transformed_frames against the frames the ISTFT needs).  The library under test is the
in-tree build, or the one PAR_HIP_LIB names (an A/B against another build of stft.hip: tools/build_variant.py --src=stft.hip)."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyaudiorestoration_amd import _dev, _lib, dropouts, fourier  # noqa: E402

N, SR = 26_460_000, 44100
GEOMS = ((512, 64), (2048, 512), (2048, 128), (8192, 1024))
HBM_BPS = 8.0e12           # MI355X HBM3E peak
ALGO_BYTES = 16.0          # per stereo sample: 2 x 4 B read, 2 x 4 B written


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
    return {"ms": float(np.median(ts)), "ms_min": float(np.min(ts))}


def rate(r, n):
    r["msamples_per_s"] = n / (r["ms"] * 1e-3) / 1e6
    r["share_hbm_roofline"] = ALGO_BYTES * n / (r["ms"] * 1e-3) / HBM_BPS
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--samples", type=int, default=N)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n = a.samples
    dev = 0
    torch.cuda.set_device(dev)
    cuda = f"cuda:{dev}"
    g = torch.Generator(device=cuda).manual_seed(3)
    t = torch.arange(n, device=cuda, dtype=torch.float64) / SR
    tone = (0.3 * torch.sin(2 * math.pi * 440.0 * t) * (1 + 0.5 * torch.sin(2 * math.pi * 0.05 * t))).to(torch.float32)
    x = (torch.stack([tone, 0.8 * torch.roll(tone, 7)], dim=1) + 0.01 * torch.randn((n, 2), generator=g, device=cuda)).contiguous()
    del t, tone
    L = _lib.lib()
    res = {"samples": n, "library": os.environ.get("PAR_HIP_LIB") or "in-tree", "algorithmic_bytes_per_stereo_sample": ALGO_BYTES}
    for fft, hop in GEOMS:
        half = fft // 2
        window_t = fourier.window_dev("blackmanharris", fft, dev)
        out = _dev.empty((n, 2), torch.float32, dev)
        r = {}
        if dropouts.fused_supported(fft, hop):
            r["fused"] = rate(timed(lambda: dropouts.max_mono_dev(x, fft, hop, fused=True, dev=dev, out=out), a.reps, dev), n)
            need = min(int(L.par_stft_frames(n + half, fft, hop)), -(-(n + fft) // hop))
            r["redundant_frame_share"] = 1.0 - need / int(L.par_maxmono_stft_transformed_frames(n, fft, hop))
            y_fused = out.clone()
        r["composed"] = rate(timed(lambda: dropouts.max_mono_dev(x, fft, hop, fused=False, dev=dev, out=out), a.reps, dev), n)
        if "fused" in r:
            peak = float(out.abs().max())
            r["fused_vs_composed_of_peak"] = max(float((y_fused[s:s + (1 << 22)].double() - out[s:s + (1 << 22)].double()).abs().max())
                                                 for s in range(0, n, 1 << 22)) / peak
            del y_fused
        # the composed route stage by stage, on buffers of its own
        state = {}

        def stage_stft():
            fms = []
            for c in (0, 1):
                xpad = torch.zeros(n + half, dtype=torch.float32, device=cuda)
                xpad[:n] = x[:, c]
                fms.append(fourier.stft_dev(xpad, fft, hop, window_t, 1, 0, dev=dev).T)
            state["fms"] = fms

        def stage_select():
            state["sel"] = dropouts.select_spectra_dev(state["fms"][0], state["fms"][1], dev)

        def stage_istft():
            for k, fm in enumerate(state["sel"]):
                out[:, k] = fourier.istft_dev(fm.T, hop, window_t, length=n, dev=dev)
        r["composed_stages"] = {"stft_x2": timed(stage_stft, a.reps, dev), "select": timed(stage_select, a.reps, dev),
                                "istft_x2": timed(stage_istft, a.reps, dev)}
        state.clear()
        # the same chain in torch on the same GPU
        try:
            xpadded = torch.zeros((2, n + half), dtype=torch.float32, device=cuda)
            xpadded[:, :n] = x.T

            def torch_chain():
                D = torch.stft(xpadded, fft, hop, window=window_t, center=True, pad_mode="reflect", return_complex=True)
                m = D.abs()
                for k, mask in enumerate((m[0] > m[1], m[0] < m[1])):
                    out[:, k] = torch.istft(torch.where(mask, D[0], D[1]), fft, hop, window=window_t, center=True, length=n)
            r["torch"] = rate(timed(torch_chain, max(2, a.reps // 2), dev), n)
            del xpadded
        except Exception as e:                                           # reported, not hidden: the figure is then "not measured"
            r["torch"] = {"not_measured": f"{type(e).__name__}: {e}"[:300]}
        torch.cuda.empty_cache()
        if "fused" in r:
            r["fused_speedup_over_composed"] = r["composed"]["ms"] / r["fused"]["ms"]
        res[f"{fft}/{hop}"] = r
        print(json.dumps({f"{fft}/{hop}": r}), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
