"""Zero-crossing flutter analysis of the reference (experiments/zerocrossing_wow.py) on the GPU, headless: the pitch of a clean
pilot tone from the spacing of its sign changes.

    res = detect_crossings("tape.flac", hop=256)                 # the script's detect_crossings, its plot calls removed
    res.times, res.freqs, res.raw_freqs                          # per crossing: the smoothed and the "raw" curve (device tensors)
    res.grid_times, res.grid_freqs                               # the smoothed curve every `hop` samples (numpy)
    curve = speed_curve(res)                                     # [[t, speed], ...] for resampling.run(speed_curve=...)

The script takes the sign changes of channel 0, their spacing as float32 half periods, pads them by `size` = about 10 ms of
crossings in reflect mode, convolves with a Hann kernel of that size and plots sr / 2 / period over the crossings' times; it stops
at "todo transform to a regularly sampled pitch curve".  Here the samples go to the device once (only the requested channel), the
sign changes are compacted there (par_zero_crossings_f64), the smoothing, the division and the time axis are one launch
(par_crossing_smooth_f64) and the regular grid is np.interp on the device (par_interp_f64).  Two crossing indices come back for
the span, and the grid if one is asked for; the per-crossing curves stay in HBM until someone reads them.  There is no CPU path.

wow_detection.ZeroCrossingTracker.trace keeps its host tail (crossing_periods_to_freqs): routing it through these kernels would
change the last bits of its results (another summation order), which is a change of its own."""
import collections

import numpy as np
import torch
from scipy.signal import get_window

from . import _dev, _lib, filters, io_ops, pipeline
from .wow_detection import zero_crossings_dev

MAX_SPAN = _lib.CROSSING_SMOOTH_MAX_SPAN
ZeroCrossingPitch = collections.namedtuple("ZeroCrossingPitch", "raw_times raw_freqs times freqs span grid_times grid_freqs")
Smoothed = collections.namedtuple("Smoothed", "xp freq raw span")


def smoothing_span(sr, first, last, n):
    """The script's `size` (experiments/zerocrossing_wow.py:22): crossings in 10 ms, int(sr / 100 / mean period), from the first
    and the last crossing index and the number n of periods between them.  The periods sum to last - first exactly (the sum
    telescopes), so the mean is (last - first) / n in float64 and only two indices are read back, never the array.  The reference
    takes np.mean of the float32 periods, which is float32 pairwise summation: its mean is off by up to about 2^-20 relative, and
    the two spans can differ only where the quotient lies that close to an integer.  A span below 1 is a pilot under 50 Hz: the
    reference's np.convolve then raises "v cannot be empty", a ValueError, and so does this."""
    span = int(float(sr) / 100 / ((int(last) - int(first)) / int(n)))
    if span < 1:
        raise ValueError(f"v cannot be empty: {n} periods over {int(last) - int(first)} samples at {sr} Hz give a smoothing span of "
                         f"{span} crossings (a pilot under 50 Hz)")
    return span


def hann_kernel(span):
    """The script's weights, win_sq / size * 2 (experiments/zerocrossing_wow.py:26-28): scipy's bits, computed on the host"""
    return get_window("hann", int(span)) / int(span) * 2


def smooth_crossings_dev(crossings_t, sr, t0=0.0, span=None, raw=False):
    """Sign-change indices (device int64, ascending) -> Smoothed(xp, freq, raw, span): xp = crossings[:n] / sr + t0 and freq =
    sr / 2 / (the Hann-smoothed periods) as device float64 tensors of n = len(crossings) - 1 values, raw = float32 sr / 2 / period
    (None unless asked for), one launch of par_crossing_smooth_f64.  span=None is smoothing_span of these crossings.  Fewer than 3
    crossings: ValueError (one period cannot be reflected)."""
    c = int(crossings_t.numel())
    if c < 3:
        raise ValueError(f"{c} zero crossings: at least 3 are needed")
    dev = _dev.device_index(crossings_t.device)
    crossings_t = crossings_t.contiguous()
    n = c - 1
    if span is None:
        first, last = crossings_t[[0, c - 1]].cpu().tolist()
        span = smoothing_span(sr, first, last, n)
    span = int(span)
    if not 1 <= span <= MAX_SPAN:
        raise ValueError(f"a smoothing span of {span} crossings is outside [1, {MAX_SPAN}]")
    kernel_t = _dev.to_dev(hann_kernel(span), torch.float64, dev)
    xp = _dev.empty(n, torch.float64, dev)
    freq = _dev.empty(n, torch.float64, dev)
    raw_t = _dev.empty(n, torch.float32, dev) if raw else None
    _lib.check(_lib.lib().par_crossing_smooth_f64(dev, _dev.ptr(crossings_t), c, _dev.ptr(kernel_t), span, float(sr), float(t0), None,
                                                  _dev.ptr(freq), _dev.ptr(xp), _dev.ptr(raw_t) if raw else None,
                                                  _dev.stream_ptr(dev)))
    return Smoothed(xp, freq, raw_t, span)


def interp_dev(x_t, xp_t, fp_t):
    """np.interp(x, xp, fp) on the device, numpy's bits (par_interp_f64) -> device float64 tensor shaped like x"""
    dev = _dev.device_index(xp_t.device)
    x_t, xp_t, fp_t = (_dev.to_dev(t, torch.float64, dev) for t in (x_t, xp_t, fp_t))
    if xp_t.numel() != fp_t.numel():
        raise ValueError("fp and xp are not of the same length.")
    out = _dev.empty(tuple(x_t.shape), torch.float64, dev)
    _lib.check(_lib.lib().par_interp_f64(dev, _dev.ptr(x_t), x_t.numel(), _dev.ptr(xp_t), _dev.ptr(fp_t), xp_t.numel(), _dev.ptr(out),
                                         _dev.stream_ptr(dev)))
    return out


def grid(n_samples, sr, hop):
    """The regular time axis: every `hop` samples from 0 to the last whole hop, in seconds"""
    return np.arange(int(n_samples) // int(hop) + 1) * (int(hop) / sr)


def detect_crossings(path_or_signal, sr=None, channel=0, band=None, order=3, hop=None, device=None):
    """experiments/zerocrossing_wow.py's detect_crossings on a file (or on a signal, numpy or device tensor, (n,) or (n, channels),
    with its sample rate) -> ZeroCrossingPitch(raw_times, raw_freqs, times, freqs, span, grid_times, grid_freqs).

    times = crossings[:n] / sr and raw_times (the same tensor), freqs the smoothed curve (float64), raw_freqs the script's "raw"
    curve (float32): device tensors, one value per period.  span is the script's `size`.  band=None filters nothing, as the
    script does (its "todo bandpass" is open); band=(lo, hi) Hz is an extension: filters.bandpass_dev of `order` first, as
    ZeroCrossingTracker does.  hop gives the script's other todo, the regularly sampled curve: grid_times = arange(n // hop + 1) *
    (hop / sr) and grid_freqs = np.interp(grid_times, times, freqs), numpy arrays (None without hop).  Only the requested channel
    is uploaded."""
    if isinstance(path_or_signal, str):
        signal, sr, _ = io_ops.read_file(path_or_signal)
    else:
        signal = path_or_signal
        if sr is None:
            raise ValueError("a signal needs its sample rate")
    if signal.ndim == 1:
        signal = signal[:, None]
    channel = int(channel)
    if signal.ndim != 2 or not 0 <= channel < signal.shape[1]:
        raise ValueError(f"channel {channel} of a signal of shape {tuple(signal.shape)}")
    dev = _dev.device_index(device if device is not None else (signal.device if isinstance(signal, torch.Tensor) and signal.is_cuda else None))
    n_samples = signal.shape[0]
    x = signal[:, channel]
    if band is None:
        x_t = _dev.to_dev(x, torch.float64, dev)
    else:
        x_t = filters.bandpass_dev(x, float(band[0]), float(band[1]), sr, order=order, dev=dev)
    crossings_t = zero_crossings_dev(x_t, dev)
    sm = smooth_crossings_dev(crossings_t, sr, 0.0, raw=True)
    grid_times = grid_freqs = None
    if hop is not None:
        grid_times = grid(n_samples, sr, hop)
        grid_freqs = interp_dev(_dev.to_dev(grid_times, torch.float64, dev), sm.xp, sm.freq).cpu().numpy()
    return ZeroCrossingPitch(sm.xp, sm.raw, sm.xp, sm.freq, sm.span, grid_times, grid_freqs)


def _host(a):
    return _dev.to_host(a) if isinstance(a, torch.Tensor) else np.asarray(a)


def speed_curve(result):
    """The pitch curve on the regular grid as [[t seconds, linear speed], ...], speed = 2 ** pipeline.trace_to_speed(grid_freqs)
    (log2 of the pitch, centred on its mean): the shape cyclic_wow.speed_curve returns, which is what
    resampling.run(speed_curve=...) takes to remove the flutter."""
    if result.grid_times is None:
        raise ValueError("no regular grid: call detect_crossings with hop")
    t = np.asarray(result.grid_times, dtype=np.float64)
    return np.stack((t, np.power(2.0, pipeline.trace_to_speed(np.asarray(result.grid_freqs, dtype=np.float64)))), axis=-1)


def report(result):
    """The figures of an analysis as a dict: the span, the mean frequency, and the peak-to-peak and RMS deviation from that mean
    in percent -- of the regular grid where there is one, else of the smoothed per-crossing curve (downloaded for it)."""
    f = np.asarray(result.grid_freqs, dtype=np.float64) if result.grid_freqs is not None else _host(result.freqs)
    mean = float(np.mean(f))
    return {"span": int(result.span), "crossings": len(result.times) + 1, "mean_hz": mean, "peak_to_peak_percent": float((np.max(f) - np.min(f)) / mean * 100.0),
            "rms_percent": float(np.sqrt(np.mean((f / mean - 1.0) ** 2)) * 100.0)}
