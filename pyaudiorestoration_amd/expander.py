"""Headless restatement of the Spectral Expander (reference expander_gui.MainWindow; defaults expander_gui.py:23-25, 35-91).

The reference takes a full dB spectrogram of every analysed channel (fft 512, hop 64: 16 bytes per input sample, twice) to read
the 13-17 kHz rows of it.  Here the band curve comes straight out of the STFT kernel (par_stft_band_db_f32: one float64 per frame
leaves the kernel); the smoothing, the per-sample gain, the split filter and the normalisation run in K_expand / K_sosfiltfilt.

    curves, t = volume_curves(signal, sr)                # on_param_changed (expander_gui.py:114-137)
    out = expand(signal, sr, curves)                     # expand (expander_gui.py:178-205)
    expand_file("tape.wav")                              # ... and the file written as tape_decompressed.wav (:206)
"""
import logging
import os

import numpy as np
import torch

from . import _dev, _lib, filters, io_ops, spectrum_flat
from .filters import make_odd

# The band curve straight out of the STFT kernel (par_stft_band_db_f32).  False: the composed path -- magnitude rows of frame
# chunks, then par_band_mean_db_f32 -- which is also what transforms above 16384 points take.
FUSED = True


def freq2bin(f, num_bins, fft_size, sr):
    """expander_gui.py:128-129"""
    return max(1, min(num_bins - 3, int(round(f * fft_size / sr))))


def smoothing_size(smoothing, sr, hop):
    """The uniform filter's window in frames (expander_gui.py:121)."""
    return make_odd(int(smoothing * sr / hop))


def analysed_channels(channel_mode, num_channels):
    """Channels spectrum_from_audio_stereo analyses (util/spectrum_flat.py:9-17): channel_map's, up to the first that the file
    lacks (the mono fallback)."""
    chans = []
    for channel in spectrum_flat.channel_map[channel_mode]:
        if channel == num_channels:
            logging.warning("not enough channels for L/R comparison  - fallback to mono")
            break
        chans.append(channel)
    return chans


def _as_2d(signal):
    return signal if signal.ndim == 2 else signal[:, None]


def volume_curves(signal, sr, fft_size=512, hop=64, channel_mode="L+R", band_lower=13000, band_upper=17000, smoothing=0.11,
                  device=None, fused=None):
    """Smoothed band-volume curves of expander_gui.on_param_changed.  signal: (n, ch) (or (n,)) float32, numpy or device tensor.
    Returns (curves, t): curves float64 (k, frames) -- one row per entry of spectrum_from_audio_stereo ([L, R], [L, L], [R, R] or
    [M, M]), numpy for numpy input and a device tensor for a tensor -- and t = arange(0, hop * frames, hop) / sr.  "Mean" is the
    mean of the per-channel band curves (the reference's band mean of the averaged dB spectra, up to rounding).  An empty band
    gives all-NaN curves (np.nanmean of an empty slice); a mono file in mode "R" raises IndexError like the reference."""
    dev = _dev.device_index(device if device is not None else (signal.device if torch.is_tensor(signal) else None))
    was_tensor = torch.is_tensor(signal)
    sig2d = _as_2d(signal)
    n, ch = sig2d.shape
    sig_t = _dev.to_dev(sig2d, torch.float32, dev)
    flat = sig_t.reshape(-1)
    frames = int(_lib.lib().par_stft_frames(n, fft_size, hop))
    num_bins = fft_size // 2 + 1
    bL = freq2bin(band_lower, num_bins, fft_size, sr)
    bU = freq2bin(band_upper, num_bins, fft_size, sr)
    chans = analysed_channels(channel_mode, ch)
    raw = _dev.empty((max(len(chans), 1), frames), torch.float64, dev)
    if bL >= bU:
        raw.fill_(float("nan"))
    else:
        for i, c in enumerate(chans):
            spectrum_flat.band_db_curve_dev(flat[c:], fft_size, hop, bL, bU, "hann", 1, ch, n, FUSED if fused is None else fused, dev,
                                            out=raw[i])
    rows = [raw[i] for i in range(len(chans))]
    if channel_mode == "Mean" and len(rows) > 1:
        rows = [(rows[0] + rows[1]) / 2]               # np.mean over the two channels
    if len(rows) < 2:
        rows.append(rows[0])                           # IndexError on an empty list, as spectrum_from_audio_stereo
    stacked = torch.stack(rows).contiguous()
    curves = torch.empty_like(stacked)
    _lib.check(_lib.lib().par_uniform_filter_nearest_f64(dev, _dev.ptr(stacked), stacked.shape[0], frames, smoothing_size(smoothing, sr, hop),
                                                          _dev.ptr(curves), _dev.stream_ptr(dev)))
    t = np.arange(0, hop * frames, hop) / sr
    return (curves if was_tensor else _dev.to_host(curves)), t


def expand(signal, sr, curves, clip_lower=-120, clip_upper=-85, transition=0, order=1, hop=64, device=None):
    """expander_gui.expand on an (n, ch) (or (n,)) float32 signal: per channel c, the curve curves[c] (the last one when there are
    fewer curves than channels) is clipped to [clip_lower, clip_upper], turned into the factor 10^((clip_upper - clipped) / 20),
    interpolated onto the samples (the curve's frame j sits at sample j * hop) and applied; with a transition frequency only the
    part above it is boosted (zero-phase Butterworth split of that order, filters.butter_bandpass_filter's design).  The result is
    normalised to a peak of 1 and returned as float32 of the input's shape: numpy for numpy, a device tensor for a tensor.

    Differences from the reference: the input is never modified (the reference writes the boosted channels into the array it
    read); a curve holding NaN (an empty analysis band) raises ValueError before any work, where the reference writes a file of
    NaN samples."""
    dev = _dev.device_index(device if device is not None else (signal.device if torch.is_tensor(signal) else None))
    L = _lib.lib()
    was_tensor = torch.is_tensor(signal)
    sig2d = _as_2d(signal)
    n, ch = sig2d.shape
    rows = [curves[c] if c < len(curves) else curves[-1] for c in range(ch)]
    cv = torch.stack([r.to(device=f"cuda:{dev}", dtype=torch.float64) if torch.is_tensor(r)
                      else _dev.to_dev(np.asarray(r, dtype=np.float64), torch.float64, dev) for r in rows]).contiguous()
    if bool(torch.isnan(cv).any()):
        raise ValueError("volume curve holds NaN (empty analysis band?): the reference would write NaN samples")
    frames = cv.shape[1]
    sig_t = _dev.to_dev(sig2d, torch.float32, dev)
    out_t = _dev.empty((n, ch), torch.float32, dev)
    stream = _dev.stream_ptr(dev)
    if transition:
        split = _dev.empty((2, ch, n), torch.float64, dev)          # boosted rows, then the channels as they are
        _lib.check(L.par_expand_gain_f32(dev, _dev.ptr(sig_t), ch, ch, n, _dev.ptr(cv), frames, hop, float(clip_lower), float(clip_upper),
                                         None, ch, _dev.ptr(split), stream))
        lp = filters.bandpass_batch_dev(split[1], 0, transition, sr, order=order, dev=dev)
        hp = filters.bandpass_batch_dev(split[0], transition, sr // 2, sr, order=order, dev=dev)
        _lib.check(L.par_sum_rows_f64_f32(dev, _dev.ptr(lp), _dev.ptr(hp), ch, n, _dev.ptr(out_t), ch, stream))
    else:
        _lib.check(L.par_expand_gain_f32(dev, _dev.ptr(sig_t), ch, ch, n, _dev.ptr(cv), frames, hop, float(clip_lower), float(clip_upper),
                                         _dev.ptr(out_t), ch, None, stream))
    scratch = _dev.empty(_lib.NORMALIZE_SCRATCH_BYTES, torch.uint8, dev)
    _lib.check(L.par_normalize_f32(dev, _dev.ptr(out_t), n * ch, _dev.ptr(scratch), stream))
    res = out_t if signal.ndim == 2 else out_t[:, 0]
    return res if was_tensor else _dev.to_host(res)


def expand_file(path, channel_mode="L+R", fft_size=512, hop=64, band_lower=13000, band_upper=17000, smoothing=0.11, clip_lower=-120,
                clip_upper=-85, transition=0, order=1, suffix="_decompressed", device=None, signal_data=None):
    """open_file + expand of the GUI: read `path` (io_ops.read_file; signal_data=(signal, sr, channels) skips the read), analyse,
    expand and write <stem><suffix>.wav (io_ops.write_file, float32 like the reference's).  Returns the written path."""
    dev = _dev.device_index(device)
    signal, sr, num_channels = io_ops.read_file(path) if signal_data is None else signal_data
    sig_t = _dev.to_dev(_as_2d(signal), torch.float32, dev)                # one upload (staged ring) for both stages
    curves, _ = volume_curves(sig_t, sr, fft_size, hop, channel_mode, band_lower, band_upper, smoothing, dev)
    out = _dev.to_host(expand(sig_t, sr, curves, clip_lower, clip_upper, transition, order, hop, dev))
    io_ops.write_file(path, out, sr, num_channels, suffix)
    return f"{os.path.splitext(path)[0]}{suffix}.wav"
