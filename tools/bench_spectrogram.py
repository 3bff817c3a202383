"""Spectrogram image timings (NOTES.md "Spectrogram image"): the peak-hold image of one channel, 2048 x 1024 mel pixels, by

  fused      par_stft_peak_image_f32 (spectrogram.peak_image_dev, fused=True): frames transformed and maximised in registers, one
             column of rows written per (column, chunk); no spectrogram stored
  composed   fourier.stft_dev mode 1 over chunks of at most 1 GiB of the frames the picture names, each maximised into the image by
             par_peak_image_f32 (fused=False): K_stft mode 1 as it has always been, so this is the yardstick
  torch      torch.stft (center, reflect) over the same chunks, abs, + 1e-7, adaptive_max_pool1d over the frames of a column and
             index_reduce(amax) over the bins of a row: the framework's own kernels, columns and rows approximated (equal splits,
             a bin in one row), for scale only

at three shapes: a 10-min 44.1 kHz overview at 4096 / 8, a 60-min 192 kHz overview at 4096 / 16, and a 10-s zoom into the latter;
then par_image_colorize_u8 alone on the 2048 x 1024 image, and spectrogram.render_file file to file (10 min of 44.1 kHz mono WAV).

    python tools/bench_spectrogram.py [--reps 10] [--json profiles/spectrogram_bench.json] [--skip-long] [--skip-files]

Protocol: the signal is synthetic noise resident in HBM.  After two warm calls of each route, fused and composed alternate for
`reps` rounds in one process, every call timed by HIP events around it; medians are reported.  Then the composed route is repeated
alone in three more series of `reps` calls: `spread_ms` is the distance between the largest and the smallest of its four medians.
`fused_not_slower` is fused median <= composed median + spread; spectrogram.FUSED follows it.  The two images are compared bit for
bit at every shape.  Algorithmic bytes: fused reads the named samples once and writes the image; composed reads them once, writes
and reads the named frames' magnitudes and writes the image."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyaudiorestoration_amd import io_ops, spectrogram  # noqa: E402

WIDTH, HEIGHT = 2048, 1024
# name, fft, overlap, sample rate, seconds, (t0, t1) or None
SHAPES = (("overview_10min_44k", 4096, 8, 44100, 600, None), ("overview_60min_192k", 4096, 16, 192000, 3600, None),
          ("zoom_10s_of_60min_192k", 4096, 16, 192000, 3600, (1000.0, 1010.0)))


def noise(n, dev):
    g = torch.Generator(device=f"cuda:{dev}").manual_seed(11)
    sig = torch.empty(n, dtype=torch.float32, device=f"cuda:{dev}")
    step = 1 << 26
    for s in range(0, n, step):
        sig[s:s + step] = 0.1 * torch.randn(min(step, n - s), generator=g, device=f"cuda:{dev}")
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


def torch_route(sig, geo, window, max_bytes=1 << 30):
    """torch.stft + amax, chunked over the named frames (frames at a chunk's seams see the chunk's own reflection: timing only)"""
    named = geo.col_hi > geo.col_lo
    first, last = int(geo.col_lo[named].min()), int(geo.col_hi[named].max())
    chunk = max(1, max_bytes // (8 * geo.bins))
    cols_per_frame = int(named.sum()) / max(1, last - first)
    row_of_bin = torch.full((geo.bins,), geo.height, dtype=torch.int64, device=sig.device)
    for r in range(geo.height - 1, -1, -1):
        row_of_bin[int(geo.row_lo[r]):int(geo.row_hi[r])] = r
    out = []
    for fa in range(first, last, chunk):
        fb = min(last, fa + chunk)
        seg = sig[fa * geo.hop:(fb - 1) * geo.hop + 1]
        S = torch.stft(seg, geo.fft_size, geo.hop, window=window, center=True, pad_mode="reflect", return_complex=True)
        mag = S.abs() / float(np.sqrt(geo.fft_size)) + 1e-7                                     # (bins, frames)
        w = max(1, int(round(mag.shape[1] * cols_per_frame)))
        pooled = torch.nn.functional.adaptive_max_pool1d(mag[None], w)[0]                       # (bins, columns of this chunk)
        img = torch.zeros((geo.height + 1, w), dtype=torch.float32, device=sig.device)
        img.index_reduce_(0, row_of_bin, pooled, "amax", include_self=True)
        out.append(img[:geo.height])
    return torch.cat(out, dim=1)


def measure(sig, sr, fft, overlap, span, reps, dev, with_torch=True):
    t0, t1 = span if span is not None else (None, None)
    geo = spectrogram.geometry(sig.shape[0], sr, fft, fft // overlap, 1, WIDTH, HEIGHT, t0=t0, t1=t1)
    fused = lambda: spectrogram.peak_image_dev(sig, sr, geo, fused=True)
    composed = lambda: spectrogram.peak_image_dev(sig, sr, geo, fused=False)
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
    named = geo.col_hi > geo.col_lo
    frames = int(geo.col_hi[named].max() - geo.col_lo[named].min())
    samples = frames * geo.hop + fft
    r = {"samples": int(sig.shape[0]), "fft_size": fft, "hop": geo.hop, "frames_total": geo.n_frames, "frames_named": frames,
         "width": WIDTH, "height": HEIGHT, "fused": stats(tf), "composed": stats(tc), "composed_alone_medians_ms": medians[1:],
         "spread_ms": spread, "ratio_composed_over_fused": float(np.median(tc) / np.median(tf)),
         "fused_not_slower": bool(np.median(tf) <= np.median(tc) + spread),
         "images_bit_identical": bool(np.array_equal(a.view(np.uint32), b.view(np.uint32))),
         "fused_algorithmic_bytes": int(samples * 4 + WIDTH * HEIGHT * 4),
         "composed_algorithmic_bytes": int(samples * 4 + 2 * frames * geo.bins * 4 + WIDTH * HEIGHT * 4)}
    if with_torch:
        window = torch.from_numpy(__import__("scipy.signal").signal.get_window("blackmanharris", fft).astype(np.float32)).to(sig.device)
        try:
            for _ in range(2):
                torch_route(sig, geo, window)
            r["torch"] = stats([once(lambda: torch_route(sig, geo, window), dev) for _ in range(max(3, reps // 2))])
        except RuntimeError as e:                   # (an operator the framework lacks on this device: recorded as not measured)
            r["torch"] = {"not_measured": str(e).splitlines()[0]}
    return r, fused()


def measure_colorize(peak, reps, dev):
    for _ in range(3):
        spectrogram.colorize_dev(peak)
    lut = spectrogram.colormap("heat")
    ts = [once(lambda: spectrogram.colorize_dev(peak, cmap=lut), dev) for _ in range(reps * 5)]
    return dict(stats(ts), width=int(peak.shape[0]), height=int(peak.shape[1]), note="includes the 1 KiB table upload")


def measure_files(reps, dev):
    sr, n = 44100, 44100 * 600
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "tape.wav")
    try:
        io_ops.write_wav_float(path, (0.1 * np.random.default_rng(0).standard_normal((n, 1))).astype(np.float32), sr)
        ts = []
        for i in range(reps + 1):
            t0 = time.perf_counter()
            spectrogram.render_file(path)
            torch.cuda.synchronize(dev)
            if i:
                ts.append((time.perf_counter() - t0) * 1e3)
        return dict(stats(ts), samples=n, sample_rate=sr, what="read + upload + image + colours + download + PNG + JSON, wall clock")
    finally:
        for name in os.listdir(tmp):
            os.remove(os.path.join(tmp, name))
        os.rmdir(tmp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--skip-long", action="store_true", help="leave the 60-minute shapes out (2.8 GB of samples)")
    ap.add_argument("--skip-files", action="store_true", help="leave render_file out")
    ap.add_argument("--skip-torch", action="store_true", help="leave the torch.stft route out")
    a = ap.parse_args()
    dev = 0
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(dev), "reps": a.reps, "FUSED_shipped": spectrogram.FUSED}
    sig, key, peak = None, None, None
    for name, fft, overlap, sr, seconds, span in SHAPES:
        if a.skip_long and seconds > 600:
            continue
        if key != (sr, seconds):
            del sig
            torch.cuda.empty_cache()
            sig, key = noise(sr * seconds, dev), (sr, seconds)
        r, peak = measure(sig, sr, fft, overlap, span, a.reps, dev, not a.skip_torch)
        res[name] = dict(r, sample_rate=sr, seconds=seconds, span=span)
        print(json.dumps({name: res[name]}), flush=True)
    del sig
    torch.cuda.empty_cache()
    res["colorize_2048x1024"] = measure_colorize(peak, a.reps, dev)
    print(json.dumps({"colorize_2048x1024": res["colorize_2048x1024"]}), flush=True)
    if not a.skip_files:
        res["render_file_10min_44k"] = measure_files(3, dev)
        print(json.dumps({"render_file_10min_44k": res["render_file_10min_44k"]}), flush=True)
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
