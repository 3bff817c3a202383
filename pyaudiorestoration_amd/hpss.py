"""Headless restatement of the harmonic / percussive separation tool (reference experiments/hpss_gui.py MainWindow.process_hpss,
parameters from util/widgets.py:927-973 HPSSWidget).

    h, p, r = separate(signal, sr)                                  # r is None for margin 1
    separate_file("take.flac", kernel=(31, 17), margin=(2.0, 3.0))  # -> take_H.wav, take_P.wav, take_R.wav

Per channel the reference zero-extends the signal by fft_size/2 (fix_length), takes a complex STFT (blackmanharris), splits it
with decompose.hpss, runs the ISTFT of both parts (length n) and, for margin != 1, forms the residual signal - (h + p).  Here the
chain is K_stft -> par_hpss_f32 -> 2 x K_istft (-> par_residual_f32) on the device, one channel at a time; FFT sizes above 16384
take the four-step STFT (par_stft_big_f32) and the scratch ISTFT, through the same par_hpss_f32.

Peak device memory: three complex spectrograms of one channel (S, H, P: 3 x 8 bytes x frames x bins, frames = (n + fft_size/2)
// hop + 1) besides the signal and the outputs; H and P are reused from channel to channel, S is freed after each.
"""
import os

import numpy as np
import torch

from . import _dev, _lib, decompose, fourier, io_ops

WINDOW = "blackmanharris"
# GUI defaults: FFT 512 (hpss_gui.py:31), overlap 4, kernels 31 / 31, power 2, margin 1 (util/widgets.py:927-973)
FFT_SIZE, OVERLAP, KERNEL, POWER, MARGIN = 512, 4, (31, 31), 2.0, 1.0


def _as_2d(signal):
    return signal if signal.ndim == 2 else signal[:, None]


def has_residual(margin):
    """process_hpss writes the residual when `margin != 1.0` (a tuple never equals 1.0)."""
    return not (np.isscalar(margin) and margin == 1.0)


def separate_dev(sig_t, fft_size=FFT_SIZE, hop=FFT_SIZE // OVERLAP, kernel=KERNEL, power=POWER, margin=MARGIN, channels=None, dev=None):
    """Device form of separate: sig_t float32 (n, ch) device tensor -> (h, p, r_or_None), float32 (n, len(channels)) tensors."""
    dev = _dev.device_index(dev if dev is not None else sig_t.device)
    win_harm, win_perc, power, margin_harm, margin_perc = decompose._check(kernel, power, margin)
    n, ch = sig_t.shape
    chans = list(range(ch)) if channels is None else [int(c) for c in channels]
    if not chans:
        raise ValueError("no channel selected")
    for c in chans:
        if not 0 <= c < ch:
            raise IndexError(f"channel {c} of a {ch}-channel signal")
    k = len(chans)
    L = _lib.lib()
    window_t = fourier.window_dev(WINDOW, fft_size, dev)
    h_out = _dev.empty((n, k), torch.float32, dev)
    p_out = _dev.empty((n, k), torch.float32, dev)
    r_out = _dev.empty((n, k), torch.float32, dev) if has_residual(margin) else None
    half = fft_size // 2
    xpad = torch.zeros(n + half, dtype=torch.float32, device=f"cuda:{dev}")          # fourier.fix_length(signal, n + fft_size // 2)
    bufs = None
    for i, c in enumerate(chans):
        xpad[:n] = sig_t[:, c]
        spec = fourier.stft_dev(xpad, fft_size, hop, window_t, 1, 0, dev=dev)         # (bins, frames) view of [frames][bins]
        H, P = decompose.hpss_dev(spec.T, win_harm, win_perc, power, margin_harm, margin_perc, dev=dev, out=bufs)
        bufs = (H, P)                                                                 # packed rows: the views are the buffers
        del spec
        h_out[:, i] = fourier.istft_dev(H.T, hop, window_t, length=n, dev=dev)
        p_out[:, i] = fourier.istft_dev(P.T, hop, window_t, length=n, dev=dev)
        if r_out is not None:
            _lib.check(L.par_residual_f32(dev, _dev.ptr(sig_t[:, c]), sig_t.stride(0), _dev.ptr(h_out[:, i]), k, _dev.ptr(p_out[:, i]), k,
                                          n, _dev.ptr(r_out[:, i]), k, _dev.stream_ptr(dev)))
    return h_out, p_out, r_out


def separate(signal, sr, fft_size=FFT_SIZE, hop=FFT_SIZE // OVERLAP, kernel=KERNEL, power=POWER, margin=MARGIN, channels=None):
    """process_hpss on an (n, ch) (or (n,)) float32 signal: (h, p, r) float32 arrays of shape (n, len(channels)) -- numpy for
    numpy input, device tensors for a tensor; a 1-D input gives 1-D results.  r is None unless margin != 1 (a scalar 1.0; any
    tuple has a residual, as in the reference).  kernel = (harmonic, percussive) median sizes or one number for both, margin
    likewise.  `sr` is not used by the separation (the file flow needs it)."""
    was_tensor = torch.is_tensor(signal)
    dev = _dev.device_index(signal.device if was_tensor else None)
    sig_t = _dev.to_dev(_as_2d(signal), torch.float32, dev).contiguous()
    outs = separate_dev(sig_t, fft_size, hop, kernel, power, margin, channels, dev)
    res = []
    for o in outs:
        if o is not None:
            o = o if signal.ndim == 2 else o[:, 0]
            o = o if was_tensor else _dev.to_host(o)
        res.append(o)
    return tuple(res)


def output_paths(path, margin=MARGIN):
    """The files process_hpss writes: io_ops.write_file(path, ..., suffix="_H" / "_P" / "_R")"""
    stem = os.path.splitext(path)[0]
    return [f"{stem}{s}.wav" for s in (("_H", "_P", "_R") if has_residual(margin) else ("_H", "_P"))]


def separate_file(path, fft_size=FFT_SIZE, overlap=OVERLAP, kernel=KERNEL, power=POWER, margin=MARGIN, device=None, signal_data=None):
    """The GUI's flow on a file: read `path` (signal_data=(signal, sr, channels) skips the read), separate every channel at
    hop = fft_size // overlap and write <stem>_H.wav, <stem>_P.wav and, for margin != 1, <stem>_R.wav (float32 WAV).  Returns
    the written paths."""
    dev = _dev.device_index(device)
    signal, sr, num_channels = io_ops.read_file(path) if signal_data is None else signal_data
    sig_t = _dev.to_dev(_as_2d(signal), torch.float32, dev).contiguous()
    outs = separate_dev(sig_t, fft_size, fft_size // overlap, kernel, power, margin, None, dev)
    for o, suffix in zip(outs, ("_H", "_P", "_R")):
        if o is not None:
            io_ops.write_file(path, _dev.to_host(o), sr, num_channels, suffix=suffix)
    return output_paths(path, margin)
